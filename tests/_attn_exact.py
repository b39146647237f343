"""Exact key-selection inputs, int64 references, case tables and checkers for
the two Llama attention kernels: attn_decode (native/kernels/decode.hip) and
attn_prefill (native/kernels/prefill.hip).  Pure CPU torch.

Why: the tolerance of test_gpu_decode's G3, 2^-8 |ref| + 4 ctx 2^-23 max|v|,
grows with ctx, and a typical key carries 1 / ctx of the weight.  Measured on
the CPU from the reference alone (G3's input recipe, pos = ctx - 1, one key
removed from the fp64 softmax, the result rounded to bf16): at ctx = 1024 a
single dropped key stays inside the bound for 183 of the 1024 keys at hd 64 and
for 232 of 1024 at hd 128; at ctx = 160 for 0 of 160.  Prefill's 2^-7 A bound
is tight (a key dropped from one row of 257 escaped in 4 of 153 tries, a key
dropped from all later rows in 1 of 65), but its table stops at 288 + 33 keys
and never has several query tiles with start > 0.

Method: scores that select, values that count.
    q  64 in one column c (per head; in prefill per row and head), 0 elsewhere
    K  0 or -64, one density per column: a key's score is exactly 0 (selected)
       or -4096 scale (deselected: -512 at hd 64, -362 at hd 128), whose
       exponential is exactly 0 in fp32 however it is computed
    V  integers from {-2, -1, 1, 2}
Every probability, every alpha and every merge weight is then exactly 0 or 1,
l is the integer count n of the selected visible keys, o their integer sum S,
and P rounded to bf16 (prefill) is exact: the kernel must store bf16(S / n).
Cache rows a kernel must not read hold K = 0 and V = 64.0 (`tempt`): such a row
would be selected if it were read.

Conditions, asserted on the reference of every case by test_attn_exact_cpu.py:
 1. levels: selected scores are exactly 0, deselected ones <= -150 (natural
    log units), key 0 is selected for every head: no row is empty.
 2. rounding: 1 <= n <= 1024 for every row, and no quotient S / n lies within
    2^-20 (relative) of a bf16 rounding midpoint.  With n <= 1024 and |S / n|
    <= 2 a quotient that is no exact tie is >= 1 / (512 n) >= 2^-19 away from
    every midpoint, and the kernel's fp32 quotient (a division, or a reciprocal
    and a multiply) is within 2^-22 of S / n: it stores the same bf16.
 3. visibility: for every (row, counted key) pair, removing the key, and
    separately counting it twice, changes one or more stored bf16 values.
    (A row with a single counted key, such as pos = 0, cannot show that key
    counted twice: the mean of one value is that value at any multiplicity.
    Removing it empties the row.  That is arithmetic, not a seed's fault, and
    the only pair the second half of the condition leaves out.)
 4. no exceptions: no case is excused from a condition; a seed that misses one
    is changed in BUMP, and the tables are fixed in this file.

Rescale coverage.  A unit (a lane group's trip, a lane group, a wave, a chunk;
in prefill a key tile) of only deselected keys holds m = -4096 scale, l > 0 and
a non-zero o, all of which must be multiplied to exactly 0 where a selected key
meets them.  Every decode case holds such `dark` units both before and after
selected ones (`decode_dark`, checked by `decode_rescale`): among the lane
groups of a wave and the waves of a chunk, and among a lane group's trips
wherever a wave makes two or more (the only online sequence; hd 64 with chunks
of 128 keys makes one).  In prefill key 0 is
in the first tile of every row (condition 1), so a dark tile can only follow
the first selected key; cases of more than 128 keys hold one.
"""
from __future__ import annotations

import dataclasses
import functools

import torch

import _prefill_ref as PR

BF, F64, I64 = torch.bfloat16, torch.float64, torch.int64
QVAL, KOFF, TEMPT_V = 64.0, -64.0, 64.0
VALUES = (-2, -1, 1, 2)
NEG_INF = float("-inf")
MAX_COUNT = 1024
MIDPOINT_MARGIN = 2.0 ** -20
BUMP: dict = {}  # case -> added to its seed (condition 4: a seed that misses a condition is changed here)


def _gen(case, salt=0):
    seed = sum(p * int(c) for p, c in zip((3, 5, 7, 11, 13, 17, 19), case)) + 1000003 * salt + BUMP.get(case, 0)
    return torch.Generator().manual_seed(seed)


def _values(shape, g):
    return torch.tensor(VALUES, dtype=I64)[torch.randint(0, 4, shape, generator=g)]


# ---- decode: the plan of attn_decode_partial_kernel ------------------------------------

def attn_chunk(ctx):
    """decode.hip's attn_chunk: 128 keys per block up to 64 blocks, then the chunks grow in steps of 64."""
    if ctx <= 128 * 64:
        return 128
    return ((ctx + 63) // 64 + 63) // 64 * 64


@dataclasses.dataclass(frozen=True)
class Plan:
    """Key k of a context lies in chunk k // c; inside it, at r = k % c, in
    block trip r // bt, wave (r % bt) // wt, load u = (r % wt) // sg of the U = 4
    in flight and lane group r % sg."""
    hd: int
    ctx: int

    @property
    def sg(self):  # lane groups of a wave: 64 / (hd / 8)
        return 512 // self.hd

    @property
    def wt(self):  # keys of one wave trip
        return 4 * self.sg

    @property
    def bt(self):  # keys of one block trip
        return 4 * self.wt

    @property
    def c(self):
        return attn_chunk(self.ctx)

    @property
    def chunks(self):
        return (self.ctx + self.c - 1) // self.c

    @property
    def trips(self):  # block trips of a full chunk (the last may be partial)
        return (self.c + self.bt - 1) // self.bt

    def grid(self, n):
        """(key, valid) as [chunks, trips, 4 waves, 4 loads, sg lane groups] for keys 0 .. n-1."""
        r = torch.arange(self.trips * self.bt).view(self.trips, 4, 4, self.sg)
        key = torch.arange(self.chunks).view(-1, 1, 1, 1, 1) * self.c + r
        return key, (r < self.c) & (key < n)

    def coords(self):
        k = torch.arange(self.ctx)
        r = k % self.c
        return k // self.c, r // self.bt, r % self.bt // self.wt, r % self.wt // self.sg, r % self.sg


@dataclasses.dataclass(frozen=True)
class DCase:
    B: int
    H: int
    KVH: int
    hd: int
    ctx: int

    def __iter__(self):
        return iter(dataclasses.astuple(self))

    @property
    def G(self):
        return self.H // self.KVH

    @property
    def plan(self):
        return Plan(self.hd, self.ctx)


def decode_id(case):
    return f"hd{case.hd}-G{case.G}-B{case.B}-ctx{case.ctx}"


BATCH_G = {64: 3, 128: 4}   # the G of the batch rows
GROWN_G = {64: 4, 128: 8}   # the G of the grown chunks
GROWN = {8192: 128, 8193: 192, 12345: 256}  # ctx -> keys per chunk
# every <HD, G> instantiation at a short and a long context
DECODE_CASES = [DCase(1, 2 * G, 2, hd, ctx) for hd in (64, 128) for G in range(1, 9) for ctx in (160, 1024)]
DECODE_CASES += [DCase(B, 2 * BATCH_G[hd], 2, hd, 160) for hd in (64, 128) for B in (2, 3, 4, 8)]  # B = 1: above
DECODE_CASES += [DCase(1, 2 * GROWN_G[hd], 2, hd, ctx) for hd in (64, 128) for ctx in GROWN]


def decode_positions(plan):
    """0, ctx - 1, the keys around the chunk boundary, and one key either side
    of a wave-trip and of a block-trip boundary, in the first chunk and in the
    last chunk that holds a whole block trip."""
    p, ctx = plan, plan.ctx
    pos = {0, ctx - 1, p.c - 1, p.c, p.c + 1}
    for base in {0, p.c * ((ctx - p.bt - 1) // p.c)}:
        pos |= {base + p.wt - 1, base + p.wt, base + p.bt - 1, base + p.bt}
    return sorted(x for x in pos if 0 <= x < ctx)


def mistake_positions(case):
    p = case.plan
    return sorted({x for x in (case.ctx - 1, p.c + 1, p.bt - 1) if 0 <= x < case.ctx})


def decode_dark(plan, x):
    """(dark, boxes): keys deselected in every column for kv heads of parity x,
    and sets of keys in each of which every column gets one selected key.

    Chunk 0, wave 0: lane group 0 holds key 0; lane group 1 + x is dark (after
    group 0).  Chunk 0, wave 3: lane group 0 is dark, before the wave's first
    selected key.  With two or more trips, a lane group's first trip is dark
    before its selected later trips (group 3 - 2x of wave 0), and a last trip
    is dark after a selected first one (x = 0: group 0 of wave 0, after key 0;
    x = 1: group 1 of wave 3).  Chunk 0, wave 1 + x is dark (after wave 0).
    With three or more chunks, chunk 1 + x is dark; with five or more, wave 0
    of chunk 3 + x is, before that chunk's first selected key; with two chunks,
    chunk 1 is dark for x = 0 only.  Every dark set depends on x, so that each
    key of decode_positions stays countable for one of the two kv heads.
    Chunk 0 holds key 0 (condition 1), so no dark chunk can come before the
    first selected key, and only the trips of a lane group are an online
    sequence: the other merges take the maximum of all their units first."""
    ck, trip, wave, _, slot = plan.coords()
    w0, w3 = (ck == 0) & (wave == 0), (ck == 0) & (wave == 3)
    dark = w0 & (slot == 1 + x)
    dark |= (ck == 0) & (wave == 1 + x)
    dark |= w3 & (slot == 0)
    boxes = [w0 & (slot == 3 - 2 * x)]
    if plan.trips >= 2:
        dark |= w0 & (slot == 3 - 2 * x) & (trip == 0)
        boxes[0] = boxes[0] & (trip >= 1)
        if x == 0:
            dark |= w0 & (slot == 0) & (trip == plan.trips - 1)
        else:
            dark |= w3 & (slot == 1) & (trip == plan.trips - 1)
            boxes.append(w3 & (slot == 1) & (trip == 0))
    if plan.chunks >= 3:
        dark |= ck == 1 + x
        if plan.chunks >= 5:
            dark |= (ck == 3 + x) & (wave == 0)
    elif plan.chunks == 2 and x == 0:
        dark |= ck == 1
    return dark, boxes


def _decode_select(plan, x, g):
    """[ctx, hd] bool: which keys each column selects.  Bernoulli with one
    density per column (sparse beyond 1024 keys, so that counts stay <= 1024),
    one forced key in every (chunk, wave) that is not dark, at every trip, load
    index and lane group, one in each box, and the keys of decode_positions."""
    ctx, hd = plan.ctx, plan.hd
    lo, hi = (0.05, 0.95) if ctx <= MAX_COUNT else (0.02, 0.05)
    dens = lo + (hi - lo) * torch.rand(hd, generator=g)
    sel = torch.rand(ctx, hd, generator=g) < dens
    dark, boxes = decode_dark(plan, x)
    ck, trip, wave, u, slot = plan.coords()
    for cls, count in ((ck * 4 + wave, plan.chunks * 4), (trip, plan.trips), (u, 4), (slot, plan.sg)):
        prio = torch.rand(ctx, hd, generator=g)  # the key of each class that draws the most is selected
        prio[dark] = -1.0
        cls = cls[:, None].expand(-1, hd)
        top = torch.full((count, hd), -1.0).scatter_reduce(0, cls, prio, "amax")
        sel |= (prio >= 0) & (prio == top.gather(0, cls))
    for box in boxes:
        prio = torch.rand(ctx, hd, generator=g)
        prio[~box | dark] = -1.0
        assert bool((box & ~dark).any())
        sel[prio.argmax(0), torch.arange(hd)] = True
    sel[decode_positions(plan)] = True  # the last key of every tested position counts, unless it is dark here
    sel[dark] = False
    sel[0] = True
    return sel


@functools.lru_cache(maxsize=2)
def decode_inputs(case):
    """q [B, H, hd], k / v [B, KVH, ctx, hd] bf16 for all ctx keys, scale, and
    sel [B, H, ctx] bool: the keys each head selects; vint [B, KVH, ctx, hd] int64."""
    B, H, KVH, hd, ctx = case
    g = _gen(case)
    cols = torch.stack([torch.randperm(hd, generator=g)[:H] for _ in range(B)])  # a column per head
    selk = torch.stack([torch.stack([_decode_select(case.plan, kh % 2, g) for kh in range(KVH)]) for _ in range(B)])
    vint = _values((B, KVH, ctx, hd), g)
    q = torch.zeros(B, H, hd)
    q.scatter_(2, cols[..., None], QVAL)
    k = torch.where(selk, 0.0, KOFF)
    kvh = torch.arange(H) // case.G
    sel = selk[:, kvh].gather(3, cols[:, :, None, None].expand(B, H, ctx, 1))[..., 0]
    return dict(q=q.to(BF), k=k.to(BF), v=vint.to(BF), scale=hd ** -0.5, sel=sel, vint=vint, cols=cols, case=case,
                refs={})


def tempt(k, v, n):
    """Copies of the caches with rows n.. holding K = 0, V = 64.0."""
    k, v = k.clone(), v.clone()
    k[:, :, n:] = 0.0
    v[:, :, n:] = TEMPT_V
    return k, v


def quotient(n, S):
    """bf16(S / n) from int64 n [...] and S [..., hd]: the quotient in fp64, one rounding.  n = 0: zeros."""
    q = S.to(F64) / n.clamp_min(1).to(F64)[..., None]
    return q.to(BF)


def decode_ref(inp, pos):
    """(n [B, H], S [B, H, hd], stored [B, H, hd] bf16) for keys 0 .. pos (all ctx keys beyond the context)."""
    case = inp["case"]
    cnt = max(0, min(pos + 1, case.ctx))
    if cnt not in inp["refs"]:
        sel = inp["sel"][:, :, :cnt].to(I64)
        n = sel.sum(-1)
        S = torch.cat([sel[:, kh * case.G:(kh + 1) * case.G] @ inp["vint"][:, kh, :cnt] for kh in range(case.KVH)], 1)
        inp["refs"][cnt] = n, S, quotient(n, S)
    return inp["refs"][cnt]


# ---- the conditions -------------------------------------------------------------------

def check_levels(scores, sel):
    """Condition 1 on fp64 scores [..., keys] and the selection they must spell."""
    assert bool(((scores == 0) == sel).all())
    assert bool((scores[~sel] <= -150.0).all())
    assert bool(sel[..., 0].all())


def midpoint_distance(n, S):
    """Smallest relative distance of a quotient S / n from a bf16 rounding midpoint (zeros excepted: they are exact)."""
    x = (S.to(F64) / n.to(F64)[..., None]).abs()
    x = x[x > 0]
    mant, _ = torch.frexp(x)
    t = mant * 256  # [128, 256): the bf16 grid is the integers
    return (((t - t.floor()) - 0.5).abs() / t).min().item()


def check_rounding(n, S):
    """Condition 2; returns (smallest count, largest count, smallest midpoint distance)."""
    assert int(n.min()) >= 1 and int(n.max()) <= MAX_COUNT, (int(n.min()), int(n.max()))
    assert float((S.to(F64) / n.to(F64)[..., None]).abs().max()) <= 2.0
    d = midpoint_distance(n, S)
    assert d >= MIDPOINT_MARGIN, d
    return int(n.min()), int(n.max()), d


def check_visibility(sel, n, S, vint):
    """Condition 3 for rows that share one kv head: sel [R, K] bool, n [R], S
    [R, hd], vint [K, hd].  A key's effect on column d depends on v[key, d]
    alone, one of four values: whether removing (adding) such a value changes
    the stored bf16 is tabulated per (row, column, value), and a matrix product
    with the one-hot values counts, per (row, key), the columns that change.
    Returns the number of (row, counted key) pairs."""
    stored = quotient(n, S)
    vals = torch.tensor(VALUES, dtype=I64)
    onehot = (vint[:, :, None] == vals).flatten(1).float()                     # [K, 4 hd]
    Su = S[:, :, None]
    gone = quotient(n - 1, (Su - vals).flatten(1)).view(*S.shape, 4) != stored[:, :, None]
    gone |= (n == 1)[:, None, None]                                             # the row would be empty
    twice = quotient(n + 1, (Su + vals).flatten(1)).view(*S.shape, 4) != stored[:, :, None]
    twice |= (n == 1)[:, None, None]                                            # the mean of one value, however often
    for name, table in (("removed", gone), ("counted twice", twice)):
        changed = table.flatten(1).float() @ onehot.t()                         # [R, K] columns that change
        blind = sel & (changed == 0)
        assert not bool(blind.any()), (name, blind.nonzero()[:4].tolist())
    return int(sel.sum())


def _order(nonempty, has, dim):
    """Along `dim`: is a dark unit (keys, none selected) before the first unit with a selected key, and one after it?"""
    dark = nonempty & ~has
    seen = has.cumsum(dim) > 0
    later = (has.flip(dim).cumsum(dim).flip(dim) - has.to(I64)) > 0
    return (dark & ~seen & later).any(dim), (dark & seen).any(dim)


def decode_rescale(inp, pos):
    """Per level, [B, H] bools (before, after): the head meets a dark unit
    before, and after, a unit with a selected key under the same parent."""
    plan = inp["case"].plan
    key, valid = plan.grid(min(pos + 1, plan.ctx))
    s = inp["sel"][:, :, key.clamp(max=plan.ctx - 1)] & valid                  # [B, H, chunks, trips, 4, 4, sg]
    v = valid.expand_as(s)
    out = {}
    # trips of a lane group; lane groups of a wave; waves of a chunk; chunks
    levels = (("trip", (5,), 3), ("group", (3, 5), 6), ("wave", (3, 5, 6), 4), ("chunk", (3, 4, 5, 6), 2))
    for name, dims, dim in levels:
        ne, has = v.any(dims, keepdim=True), s.any(dims, keepdim=True)
        b, a = _order(ne, has, dim)
        out[name] = (b.flatten(2).any(2), a.flatten(2).any(2))
    return out


def decode_coverage(inp):
    """At pos = ctx - 1, for every head: a counted key in every (chunk, wave)
    that is not dark for its kv head, at every trip, load index and in every lane group."""
    case = inp["case"]
    plan = case.plan
    ck, trip, wave, u, slot = plan.coords()
    pair = ck * 4 + wave
    for h in range(case.H):
        dark, _ = decode_dark(plan, (h // case.G) % 2)
        lit = torch.zeros(plan.chunks * 4, dtype=torch.bool).index_fill_(0, pair[~dark], True)
        for b in range(case.B):
            s = inp["sel"][b, h]
            got = torch.zeros_like(lit).index_fill_(0, pair[s], True)
            assert torch.equal(got, lit), (b, h)
            assert u[s].unique().numel() == 4 and slot[s].unique().numel() == plan.sg, (b, h)
            assert trip[s].unique().numel() == plan.trips, (b, h)
    # the last key of every tested position is counted by a head of every batch row
    assert bool(inp["sel"][:, :, decode_positions(plan)].any(1).all())


# ---- decode: the kernel's split in torch, with mistakes to switch on --------------------

def _exp_diff(a, b):
    """exp(a - b), 0 where a is the empty maximum (decode.hip's exp_diff)."""
    safe = torch.where(b == NEG_INF, torch.zeros_like(b), b)
    return torch.where(a == NEG_INF, torch.zeros_like(a), torch.exp(a - safe))


def _last(key, valid, dims):
    """The last valid key of every unit spanned by `dims` of the grid."""
    top = torch.where(valid, key, -1).amax(dims, keepdim=True)
    return valid & (key == top)


LEVEL_DIMS = {"chunk": (1, 2, 3, 4), "wave": (1, 3, 4), "trip": (3, 4)}
MERGES = ("trip", "group", "wave", "chunk")
MISTAKES = ([dict(drop=lv) for lv in LEVEL_DIMS] + [dict(twice=lv) for lv in LEVEL_DIMS]
            + [dict(unscaled=(what, lv)) for what in "lo" for lv in MERGES]
            + [dict(mask_shift=1), dict(mask_shift=-1), dict(wrong_gqa=True)])


def mistake_id(m):
    (name, val), = m.items()
    return name + "-" + ("-".join(val) if isinstance(val, tuple) else str(val))


def emulate_decode(q, k, v, pos, scale, drop=None, twice=None, unscaled=None, mask_shift=0, wrong_gqa=False,
                   info=None):
    """attn_decode in torch, split as the kernel splits it: chunk -> wave ->
    lane group -> trip, each lane group an online softmax over its trips, the
    groups of a wave merged by the xor butterfly, the waves in wave order, the
    chunks by the combine; fp32 throughout, one rounding to bf16.

    drop / twice = "chunk" | "wave" | "trip": the last key of every such unit is
    left out / counted twice.  unscaled = ("l" | "o", merge): that quantity is
    not multiplied by its weight at that merge.  mask_shift = +1 / -1: one key
    more / fewer.  wrong_gqa: head h reads kv head h % KVH.  info["hit"] says
    whether the mistake touched anything that counts (a counted key, a non-zero
    l or o under a weight that is not 1)."""
    B, H, hd = q.shape
    KVH, ctx = k.shape[1], k.shape[2]
    plan = Plan(hd, ctx)
    heads = torch.arange(H) % KVH if wrong_gqa else torch.arange(H) // (H // KVH)
    n = max(0, min(pos + 1, ctx))
    n = max(0, min(n + mask_shift, ctx))
    key, valid = plan.grid(n)
    keyc = key.clamp(max=ctx - 1)
    qs = q.float() * torch.tensor(scale, dtype=torch.float32)
    s_all = torch.einsum("bhd,bjkd->bhjk", qs, k.float())[:, torch.arange(H), heads]
    s = s_all[:, :, keyc]                                                       # [B, H, chunks, trips, 4, 4, sg]
    vv = v.float()[:, :, keyc]                                                  # [B, KVH, ..., hd]
    mult = torch.ones(key.shape)
    hit = bool((heads != torch.arange(H) // (H // KVH)).any())
    if mask_shift:  # a key more: it is there; a key fewer: some head counted it
        seen = max(0, min(pos + 1, ctx))
        hit = n > seen or (n < seen and bool((s_all[:, :, n] == 0).any()))
    if drop:
        gone = _last(key, valid, LEVEL_DIMS[drop])
        hit = bool(((s == 0) & gone).any())
        valid = valid & ~gone
    if twice:
        again = _last(key, valid, LEVEL_DIMS[twice])
        hit = bool(((s == 0) & again).any())
        mult = mult + again.float()
    s = s.masked_fill(~valid, NEG_INF)

    def weights(level, a, l, o):
        """(weight for l, weight for o) at a merge, the mistake applied."""
        nonlocal hit
        al = ao = a
        if unscaled and unscaled[1] == level:
            if unscaled[0] == "l":
                hit = hit or bool(((a != 1) & (l != 0)).any())
                al = torch.ones_like(a)
            else:
                hit = hit or bool(((a != 1)[..., None] & (o != 0)).any())
                ao = torch.ones_like(a)
        return al, ao[..., None]

    shape = (B, H, plan.chunks, 4, plan.sg)
    m, l, o = torch.full(shape, NEG_INF), torch.zeros(shape), torch.zeros(*shape, hd)
    for t in range(plan.trips):
        st = s[:, :, :, t]                                                      # [B, H, chunks, 4, 4 loads, sg]
        mx = torch.maximum(m, st.amax(-2))
        al, ao = weights("trip", _exp_diff(m, mx), l, o)
        p = _exp_diff(st, mx.unsqueeze(-2)) * mult[:, t]
        l = l * al + p.sum(-2)
        o = o * ao + (p[..., None] * vv[:, heads, :, t]).sum(-3)
        m = mx
    off = 1
    while off < plan.sg:                                                        # the lane groups of a wave
        perm = torch.arange(plan.sg) ^ off
        m2, l2, o2 = m[..., perm], l[..., perm], o[..., perm, :]
        mx = torch.maximum(m, m2)
        a1l, a1o = weights("group", _exp_diff(m, mx), l, o)
        a2l, a2o = weights("group", _exp_diff(m2, mx), l2, o2)
        m, l, o = mx, l * a1l + l2 * a2l, o * a1o + o2 * a2o
        off *= 2
    m, l, o = m[..., 0], l[..., 0], o[..., 0, :]                                # [B, H, chunks, 4]
    for level, dim in (("wave", 3), ("chunk", 2)):
        mx = m.amax(dim, keepdim=True)
        al, ao = weights(level, _exp_diff(m, mx), l, o)
        l, o, m = (l * al).sum(dim), (o * ao).sum(dim), mx.squeeze(dim)
    out = torch.where(l[..., None] > 0, o / l[..., None].clamp_min(1e-30), o)
    if info is not None:
        info["hit"] = hit
    return out.to(BF)


# ---- prefill: (B, H, KVH, hd, S, start, ctx) ----------------------------------------------

PREFILL_SHAPES = [(1, 300, 212), (2, 129, 64), (1, 257, 63), (1, 1, 1023), (1, 640, 1408)]
PREFILL_CASES = []
for _hd in (64, 128):
    for _G in (1, 4, 8):
        for _B, _S, _start in PREFILL_SHAPES:
            _slack = 5 * (len(PREFILL_CASES) % 2)  # the cache ends at the last token in every other case
            PREFILL_CASES.append((_B, 2 * _G, 2, _hd, _S, _start, _start + _S + _slack))
# the S_AT_ZERO edges, once each
PREFILL_CASES += [(1, 8, 2, 64, 1, 0, 1), (1, 8, 2, 128, 17, 0, 22), (1, 8, 2, 64, 65, 0, 65),
                  (1, 8, 2, 128, 129, 0, 134)]

prefill_id = PR.case_id


def prefill_dark_tile(case, kh):
    """The key tile (of 64) that is deselected in every column for kv head kh:
    tile 1 + kh % 2, or tile 1, whichever ends before the last key; else None."""
    B, H, KVH, hd, S, start, ctx = case
    for t in (1 + kh % 2, 1):
        if 64 * t + 64 <= start + S - 1:
            return t
    return None


@functools.lru_cache(maxsize=2)
def prefill_inputs(case):
    """q [B, S, H, hd], k / v [B, KVH, ctx, hd] bf16 (rows >= start + S tempt),
    scale, selk [B, KVH, start + S, hd] bool, vint and the column of each (b, s, h)."""
    B, H, KVH, hd, S, start, ctx = case
    nk = start + S
    g = _gen(case, 1)
    cols = torch.randint(0, hd, (B, S, H), generator=g)
    lo, hi = (0.05, 0.95) if nk <= MAX_COUNT else (0.05, 0.4)
    dens = lo + (hi - lo) * torch.rand(B, KVH, 1, hd, generator=g)
    selk = torch.rand(B, KVH, nk, hd, generator=g) < dens
    for kh in range(KVH):
        t = prefill_dark_tile(case, kh)
        if t is not None:
            selk[:, kh, 64 * t:64 * t + 64] = False
    selk[:, :, 0] = True
    vint = _values((B, KVH, nk, hd), g)
    q = torch.zeros(B, S, H, hd)
    q.scatter_(3, cols[..., None], QVAL)
    k = torch.zeros(B, KVH, ctx, hd)
    v = torch.full((B, KVH, ctx, hd), TEMPT_V)
    k[:, :, :nk] = torch.where(selk, 0.0, KOFF)
    v[:, :, :nk] = vint.float()
    return dict(q=q.to(BF), k=k.to(BF), v=v.to(BF), scale=hd ** -0.5, selk=selk, vint=vint, cols=cols, case=case)


def prefill_sel(inp, b, kh):
    """[G, S, start + S] bool for the query heads of kv head kh: row s of head g
    counts key j when its column selects it and j <= start + s."""
    B, H, KVH, hd, S, start, ctx = inp["case"]
    G = H // KVH
    cols = inp["cols"][b, :, kh * G:(kh + 1) * G].t()                           # [G, S]
    sel = inp["selk"][b, kh].t()[cols]                                          # [G, S, keys]
    return sel & (torch.arange(start + S)[None, :] <= (start + torch.arange(S))[:, None])


def prefill_ref(inp):
    """(n [B, S, H], S [B, S, H, hd], stored [B, S, H, hd] bf16)."""
    if "ref" in inp:
        return inp["ref"]
    B, H, KVH, hd, S, start, ctx = inp["case"]
    G = H // KVH
    n = torch.zeros(B, S, H, dtype=I64)
    tot = torch.zeros(B, S, H, hd, dtype=I64)
    for b in range(B):
        for kh in range(KVH):
            sel = prefill_sel(inp, b, kh).to(I64)
            n[b, :, kh * G:(kh + 1) * G] = sel.sum(-1).t()
            sums = sel.reshape(G * S, -1) @ inp["vint"][b, kh]
            tot[b, :, kh * G:(kh + 1) * G] = sums.view(G, S, hd).transpose(0, 1)
    inp["ref"] = n, tot, quotient(n, tot)
    return inp["ref"]
