"""Shared by test_select_cpu.py and test_gpu_select.py: the case table of the
token-selection kernels (vgpu.ops.select), an fp64 reference of their
definition on the CPU, an emulation of the kernels' chunked split, and the
mutants that show the table notices a wrong kernel.

A case is one set of logits [B, V] and `calls` consecutive select calls from
step `s0` on; the result is the state afterwards (out, next_tok, step, pos).

Definition (see native/kernels/select.hip).  Ordering: by value with +0 == -0,
NaN below -inf, ties to the lowest index.  Greedy takes its first element.
Sampling: c_0 .. c_{k-1} its first k; l[c_0] not finite -> c_0; w_j =
exp((l[c_j] - l[c_0]) / T) (0 for NaN), W_k = sum w; nucleus = smallest m >= 1
with sum_{j<m} w_j >= top_p W_k; token c_j for the smallest j < m with
sum_{i<=j} w_i > u W_m, else c_{m-1}.  Advance: s outside [0, T) writes
nothing; a row whose out[b, s-1] == eos >= 0 (s > 0) gets eos; out[b, s] =
next_tok[b] = token; step += 1, pos += 1.
"""
import functools

import numpy as np
import torch

BF = torch.bfloat16
CHUNK = 2048  # vgpu_select_chunk (the GPU file asserts it)
VOCAB = 128256
BIG = 65 * CHUNK + 8  # beyond 64 chunks
BATCHES = (1, 2, 3, 4, 8)
GUARD = -77  # what out / next_tok hold where nothing was written
MUTANTS = ("tie_high", "ge5", "gt4", "no_temp", "p_of_wm", "nan_first", "pos_zero_gt", "rows_swapped", "u_prev",
           "eos_not_sticky")


def f32(x) -> float:
    return float(np.float32(x))


def below(x) -> float:
    return float(np.nextafter(np.float32(x), np.float32(-np.inf)))


def above(x) -> float:
    return float(np.nextafter(np.float32(x), np.float32(np.inf)))


# ---- the fp64 reference -----------------------------------------------------------------

def ordering(x: np.ndarray, k: int, mut=()) -> np.ndarray:
    """The first k indices of the fp64 row x in the ordering (mutated by `mut`)."""
    nan = np.isnan(x)
    idx = np.arange(x.size)
    keys = [-idx if "tie_high" in mut else idx]
    if "pos_zero_gt" in mut:
        keys.append(np.signbit(x).astype(np.int64))
    keys.append(-np.where(nan, 0.0, x))
    keys.append(-nan.astype(np.int64) if "nan_first" in mut else nan.astype(np.int64))
    return np.lexsort(tuple(keys))[:k]


def first_index(rows: torch.Tensor) -> np.ndarray:
    """ordering(row, 1)[0] for every row of [R, V] at once."""
    x = rows.double()
    nan = x.isnan()
    val = torch.where(nan, torch.full_like(x, -np.inf), x)
    hit = (val == val.max(dim=1, keepdim=True).values) & ~nan
    return torch.where(hit.any(1), hit.to(torch.uint8).argmax(1), torch.zeros(x.shape[0], dtype=torch.long)).numpy()


def choose_ref(x: np.ndarray, c: np.ndarray, T: float, top_p: float, u: float, mut=()):
    """(token, nucleus size m, rank j of the token) by the definition, in fp64; c = ordering(x, top_k, mut)."""
    l = x[c]
    if not np.isfinite(l[0]):
        return int(c[0]), 1, 0
    with np.errstate(invalid="ignore"):
        w = np.exp((l - l[0]) / (1.0 if "no_temp" in mut else T))
    w[np.isnan(l)] = 0.0
    cum = np.cumsum(w)
    want = top_p * cum if "p_of_wm" in mut else top_p * cum[-1]
    ok = np.nonzero(cum > want if "gt4" in mut else cum >= want)[0]
    m = int(ok[0]) + 1 if ok.size else cum.size
    draw = u * cum[m - 1]
    ok = np.nonzero(cum[:m] >= draw if "ge5" in mut else cum[:m] > draw)[0]
    j = int(ok[0]) if ok.size else m - 1
    return int(c[j]), m, j


# ---- the kernels' own route, emulated: 16-bit keys, per-chunk lists, fp32 sums ----------

def order_keys(bits: np.ndarray) -> np.ndarray:
    b = bits.astype(np.int64)
    b = np.where(b == 0x8000, 0, b)
    key = np.where(b & 0x8000, ~b & 0xFFFF, b | 0x8000)
    return np.where((bits.astype(np.int64) & 0x7FFF) > 0x7F80, 0, key)


def key_values(key: np.ndarray) -> np.ndarray:
    bits = np.where(key & 0x8000, key & 0x7FFF, ~key & 0xFFFF).astype(np.uint32)
    return (bits << 16).view(np.float32)


def emul_candidates(bits: np.ndarray, k: int, chunk: int = CHUNK):
    """(keys, indices) of the row's first k: each chunk's own first k, then the first k of those lists."""
    V = bits.size
    comp = (order_keys(bits) << 32) | (0xFFFFFFFF - np.arange(V, dtype=np.int64))
    chunks = -(-V // chunk)
    pad = np.full(chunks * chunk, -1, dtype=np.int64)
    pad[:V] = comp
    pad = pad.reshape(chunks, chunk)
    if k == 1:
        top = pad.max(axis=1).max(keepdims=True)
    else:
        lists = -np.sort(-pad, axis=1)[:, :k].reshape(-1)
        top = -np.sort(-lists[lists >= 0])[:k]
    return top >> 32, 0xFFFFFFFF - (top & 0xFFFFFFFF)


def emul_draw(key: np.ndarray, idx: np.ndarray, T: float, top_p: float, u: float) -> int:
    """The draw among the candidates as the kernel makes it: fp32, sums in candidate order."""
    if key[0] == 0 or not np.isfinite(key_values(key[:1])[0]):
        return int(idx[0])
    one = np.float32
    l = key_values(np.where(key == 0, 0x8000, key))
    with np.errstate(invalid="ignore"):
        w = np.exp((l - l[0]) / one(T)).astype(one)
    w[key == 0] = 0
    Wk = one(0)
    for x in w:
        Wk = one(Wk + x)
    want = one(one(top_p) * Wk)
    Wm, m = one(0), 0
    while True:
        Wm = one(Wm + w[m])
        m += 1
        if m >= w.size or Wm >= want:
            break
    draw = one(one(u) * Wm)
    acc = one(0)
    for j in range(m):
        acc = one(acc + w[j])
        if acc > draw:
            return int(idx[j])
    return int(idx[m - 1])


# ---- a case, run ------------------------------------------------------------------------

def case(name, logits, *, greedy=True, top_k=1, temperature=1.0, top_p=1.0, u=None, T=None, s0=0, calls=None, pos0=11,
         eos=-1, out0=None):
    logits = logits.to(BF).contiguous()
    B = logits.shape[0]
    if u is not None:
        u = torch.as_tensor(np.asarray(u, dtype=np.float32)).reshape(-1, B).contiguous()
        T = u.shape[0] if T is None else T
    T = 1 if T is None else T
    if out0 is None:
        out0 = torch.full((B, T), GUARD, dtype=torch.int64)
    return dict(name=name, logits=logits, greedy=greedy, top_k=top_k, temperature=f32(temperature), top_p=f32(top_p),
                u=u, T=T, s0=s0, calls=T if calls is None else calls, pos0=pos0, eos=eos,
                out0=torch.as_tensor(out0, dtype=torch.int64).reshape(B, T).clone())


def simulate(c, mut=(), emulate=False):
    """The state after the case's calls: by the fp64 reference (mutated by
    `mut`), or by the emulation of the kernels' route."""
    B, T = c["logits"].shape[0], c["T"]
    out, nxt = c["out0"].clone(), torch.full((B, 1), GUARD, dtype=torch.int64)
    step, pos = c["s0"], c["pos0"]
    rows64 = c["logits"].double().numpy()
    bits = c["logits"].view(torch.int16).numpy().view(np.uint16)
    k = 1 if c["greedy"] else c["top_k"]
    if c["greedy"] and not mut and not emulate:
        fast = first_index(c["logits"])
    elif emulate:
        cands = [emul_candidates(bits[b], k) for b in range(B)]
    else:
        cands = [ordering(rows64[b], k, mut) for b in range(B)]
    for _ in range(c["calls"]):
        s = step
        if s < 0 or s >= T:
            continue
        toks = []
        for b in range(B):
            ub = 0.0
            if not c["greedy"]:
                ub = float(c["u"][max(s - 1, 0) if "u_prev" in mut else s, b])
            if c["greedy"]:
                t = int(fast[b]) if not mut and not emulate else int(cands[b][1][0] if emulate else cands[b][0])
            elif emulate:
                t = emul_draw(*cands[b], c["temperature"], c["top_p"], ub)
            else:
                t = choose_ref(rows64[b], cands[b], c["temperature"], c["top_p"], ub, mut)[0]
            toks.append(t)
        if "rows_swapped" in mut:
            toks = toks[::-1]
        for b, t in enumerate(toks):
            if c["eos"] >= 0 and s > 0 and int(out[b, s - 1]) == c["eos"] and "eos_not_sticky" not in mut:
                t = c["eos"]
            out[b, s] = t
            nxt[b, 0] = t
        step, pos = s + 1, pos + 1
    return dict(out=out, next_tok=nxt, step=step, pos=pos)


def expected(c):
    if "want" not in c:
        c["want"] = simulate(c)
    return c["want"]


def same(a, b) -> bool:
    return (torch.equal(a["out"], b["out"]) and torch.equal(a["next_tok"], b["next_tok"])
            and a["step"] == b["step"] and a["pos"] == b["pos"])


# ---- the table --------------------------------------------------------------------------

def _noise(g, R, V):
    """Rows of distinct-looking bf16 values in (-9, -1): below everything a case plants."""
    return (-1.0 - 8.0 * torch.rand(R, V, generator=g)).to(BF)


def _batches(rows):
    """Cut a list of rows into batches of the supported sizes, cycling through them; the tail repeats rows."""
    out, i, n = [], 0, 0
    while i < len(rows):
        B = BATCHES[n % len(BATCHES)]
        take = [rows[(i + j) % len(rows)] for j in range(B)]
        out.append(torch.stack(take))
        i, n = i + B, n + 1
    return out


def greedy_vocabs():
    return [8, 16, CHUNK - 8, CHUNK, CHUNK + 8, 3 * CHUNK + 8, VOCAB]


def _greedy_rows(V, g):
    edges = list(range(CHUNK, V, CHUNK))
    spots = sorted({p for p in [0, 7, 8 % V, V - 1] + [e - 1 for e in edges] + edges if 0 <= p < V})
    rows = []
    noise = _noise(g, len(spots) + 8, V)
    for r, p in enumerate(spots):  # the maximum at p
        noise[r, p] = 100.0
        rows.append(noise[r])
    r = len(spots)
    lo, hi = 5 % V, V - 3  # equal maxima: in two chunks when there are two; the lower index wins
    noise[r, lo] = noise[r, hi] = 50.0
    rows.append(noise[r])
    noise[r + 1].fill_(-1.0)  # +0 against -0: equal, the lower index wins
    noise[r + 1, 3], noise[r + 1, V - 2] = -0.0, 0.0
    rows.append(noise[r + 1])
    noise[r + 2].fill_(-1.0)
    noise[r + 2, 3], noise[r + 2, V - 2] = 0.0, -0.0
    rows.append(noise[r + 2])
    rows.append(torch.full((V,), -np.inf, dtype=BF))
    rows.append(torch.full((V,), np.nan, dtype=BF))
    mid = V // 2  # a NaN on each side of the maximum
    noise[r + 3, mid], noise[r + 3, mid - 1], noise[r + 3, mid + 1] = 100.0, np.nan, np.nan
    rows.append(noise[r + 3])
    noise[r + 4, V - 4], noise[r + 4, 2], noise[r + 4, V - 1] = np.inf, 300.0, 300.0  # +inf beats finite values
    rows.append(noise[r + 4])
    row = torch.full((V,), np.nan, dtype=BF)  # NaN ranks below -inf
    row[V - 3] = row[V - 2] = -np.inf
    rows.append(row)
    return rows


def _planted(g, B, V, values, extra_at_cut):
    """[B, V] noise with `values` at scattered places, both sides of chunk
    edges among them, different in every row, and `extra_at_cut` more copies of
    the last value: of its places only the lowest may be taken for it."""
    logits = _noise(g, B, V)
    vals = list(values) + [values[-1]] * extra_at_cut
    forced = [p for e in range(CHUNK, V, CHUNK) for p in (e - 1, e)] + [0, V - 1]
    for b in range(B):
        spots = [forced[i] for i in torch.randperm(len(forced), generator=g).tolist()][:max(len(vals) // 2, 1)]
        while len(spots) < len(vals):
            p = int(torch.randint(0, V, (1,), generator=g))
            if p not in spots:
                spots.append(p)
        for i, v in zip(torch.randperm(len(vals), generator=g).tolist(), vals):
            logits[b, spots[i]] = v
    return logits


GRADED = [2.0, 1.75, 1.5, 1.5, 1.25, 1.0, 0.75, 0.5]  # bf16 values; one tie inside, one at the cut


def _graded_probes(T):
    """For the GRADED candidates at temperature T: [(top_p, m, [u_0 .. u_{m-1}])],
    top_p at midpoints between consecutive cumulative masses (and 1), u at the
    midpoint of each nucleus member's interval, all rounded to fp32."""
    w = np.exp((np.array(GRADED) - GRADED[0]) / T)
    cum = np.concatenate([[0.0], np.cumsum(w)])
    out = []
    for m in range(1, len(GRADED) + 1):
        top_p = 1.0 if m == len(GRADED) else f32((cum[m - 1] + cum[m]) / 2 / cum[-1])
        out.append((top_p, m, [f32((cum[j] + cum[j + 1]) / 2 / cum[m]) for j in range(m)]))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    g = torch.Generator().manual_seed(2024)
    tab = []
    # greedy: every V, the rows cut into batches of every size
    for V in greedy_vocabs():
        for n, logits in enumerate(_batches(_greedy_rows(V, g))):
            tab.append(case(f"greedy V{V} #{n}", logits))
    # top_k = 1 is greedy whatever u says
    for V in (16, CHUNK + 8):
        for n, logits in enumerate(_batches(_greedy_rows(V, g))[:5]):
            B = logits.shape[0]
            tab.append(case(f"top1 V{V} #{n}", logits, greedy=False, top_k=1, temperature=0.75, top_p=0.25,
                            u=torch.rand(3, B, generator=g).numpy()))
    # uniform: k equal maxima (every weight 1), more than k of them in the row
    V, n = 3 * CHUNK + 8, 0
    for k in (1, 2, 8, 64):
        B = BATCHES[n % len(BATCHES)]
        n += 1
        logits = _planted(g, B, V, [5.0] * k, 3)
        us = [v for j in range(k) for v in ([j / k] if j == 0 else [below(j / k), j / k])]  # c_{j-1} | c_j
        tab.append(case(f"uniform k{k} u", logits, greedy=False, top_k=k, temperature=0.5,
                        u=np.repeat(np.array(us, dtype=np.float32)[:, None], B, axis=1)))
        ms = range(1, k + 1) if k <= 8 else (1, 2, 31, 32, 33, 63, 64)
        for m in ms:
            for top_p, keep in [(m / k, m)] + ([(above(m / k), m + 1)] if m < k else []):
                us, rows = [(j + 0.5) / keep for j in range(keep)], min(B, 1 + m % 2)
                tab.append(case(f"uniform k{k} p{top_p!r}", logits[:rows], greedy=False, top_k=k, temperature=2.0,
                                top_p=top_p, u=np.repeat(np.array(us, dtype=np.float32)[:, None], rows, axis=1)))
    # graded: a short list of values, three temperatures
    for T in (0.5, 1.0, 2.0):
        B = BATCHES[n % len(BATCHES)]
        n += 1
        logits = _planted(g, B, V, GRADED, 2)
        for top_p, m, us in _graded_probes(T):
            tab.append(case(f"graded T{T} m{m}", logits, greedy=False, top_k=len(GRADED), temperature=T, top_p=top_p,
                            u=np.repeat(np.array(us, dtype=np.float32)[:, None], B, axis=1)))
    # the Llama-3 vocabulary through the sampler: 63 chunks, the last one short
    logits = _planted(g, 2, VOCAB, [5.0] * 64, 3)
    tab.append(case("uniform V128256 k64", logits, greedy=False, top_k=64, temperature=1.0,
                    u=np.repeat(np.array([(j + 0.5) / 64 for j in range(64)], dtype=np.float32)[:, None], 2, axis=1)))
    # 66 chunks: more lists than the final select keeps in LDS, so it reads them in place
    logits = _planted(g, 1, BIG, [5.0] * 64, 3)
    tab.append(case(f"uniform V{BIG} k64", logits, greedy=False, top_k=64, temperature=1.0,
                    u=np.array([(j + 0.5) / 64 for j in range(64)], dtype=np.float32)))
    logits = _planted(g, 1, VOCAB, GRADED, 2)
    top_p, m, us = _graded_probes(1.0)[5]
    tab.append(case("graded V128256", logits, greedy=False, top_k=len(GRADED), temperature=1.0, top_p=top_p, u=us))
    # non-finite values through the sampler: a non-finite l[c_0] gives c_0 whatever u says; -inf and NaN
    # candidates below a finite c_0 weigh 0
    rows = torch.stack([torch.full((V,), np.nan, dtype=BF), torch.full((V,), -np.inf, dtype=BF), _noise(g, 1, V)[0],
                        torch.full((V,), -np.inf, dtype=BF), torch.full((V,), np.nan, dtype=BF),
                        torch.full((V,), np.nan, dtype=BF), torch.full((V,), -np.inf, dtype=BF), _noise(g, 1, V)[0]])
    rows[2, CHUNK], rows[2, 9] = np.inf, 7.0
    rows[3, CHUNK - 1], rows[3, 2 * CHUNK], rows[3, 4] = 1.0, 1.0, np.nan  # two finite, then six -inf
    rows[4, 10], rows[4, 3000] = 2.0, 2.0                                   # two finite, then six NaN
    rows[5, 77] = -np.inf                                                   # c_0 is the -inf
    rows[6, V - 1] = -3.0                                                   # one finite, then seven -inf
    u = torch.rand(4, 8, generator=g).numpy()
    u[0], u[1] = 0.25, 0.75
    tab.append(case("sample non-finite", rows, greedy=False, top_k=8, temperature=1.0, u=u))
    # advance
    base = _batches(_greedy_rows(CHUNK + 8, g))
    two, three = base[1], base[2]
    tab.append(case("advance one call", three, T=5, s0=2, calls=1, pos0=17))
    tab.append(case("advance three calls", two, T=4, s0=0, calls=3, pos0=0))
    tab.append(case("advance s = T", two, T=3, s0=3, calls=1))
    tab.append(case("advance s = -1", two, T=3, s0=-1, calls=1))
    tab.append(case("advance s = T, sampling", two, greedy=False, top_k=4, u=np.full((3, 2), 0.5), s0=3, calls=1))
    tab.append(case("eos sticky on row 0", two, T=3, s0=1, calls=2, eos=9, out0=[[9, GUARD, GUARD], [4, GUARD, GUARD]]))
    tab.append(case("eos sticky on row 1, sampling", two, greedy=False, top_k=2, u=np.full((3, 2), 0.5), s0=2, calls=1,
                    eos=0, out0=[[GUARD, 1, GUARD], [GUARD, 0, GUARD]]))
    tab.append(case("eos at step 0 selects", two, T=2, s0=0, calls=2, eos=9, out0=[[9, 9], [9, 9]]))
    tab.sort(key=lambda c: c["logits"].numel())  # a mutant meets the small cases first
    return tab
