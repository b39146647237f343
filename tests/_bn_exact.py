"""Exact-integer inputs, high-precision references and a plan mirror for the
BatchNorm kernels (native/kernels/bn_nhwc.hip).  Pure CPU torch; the library is
not imported here.

Forward (statistics reduced by the kernels): x[r, c] = offset_c + d[r, c] with
integer offsets up to +-200 and |d| <= 8, so x is exact in bf16 and every
shifted term x - x0, its square and every fp32 partial sum is an integer below
2**24, exact in any order; the kernels' fp64 merge is exact too.  Mean and
invstd are then one fp64 division / square root away from the int64 sums, and a
single lost or doubled row moves them by >= 16 fp32 ulp (proved on the CPU by
tests/test_bn_exact_cpu.py), against a 1-ulp assertion.

Backward and the two *_partials entry points: the saved statistics are inputs,
so they are integers / powers of two and every sum is exact: d-gamma and d-beta
must EQUAL the int64 reference.  The statistics a convolution's epilogue forms
(conv_gemm.hip, vgpu_conv2d_nhwc_bn) are sums of exact integers per 64-row
group and must EQUAL theirs too.

The plan mirror (plain_kind, make_plan, fused_grid, fused_ok) restates the
host-side choices of bn_nhwc.hip so that cases can be named by the branch they
reach; the GPU tests hold it against vgpu_bn_workspace.
"""
from __future__ import annotations

import dataclasses
import functools

import torch

from _exact import FP32_EXACT, I64, gen, nonzero_ints, signs

BF = torch.bfloat16
F32 = torch.float32
F64 = torch.float64
ACT = {"none": 0, "relu": 1, "relu6": 2}

# ---- the plan mirror ------------------------------------------------------------------
THREADS = 256          # reduction workgroup
UNROLL = 4             # rows in flight per thread (8 via set_tuning)
MAX_CHUNK = 512        # channels per reduction workgroup
TARGET_BLOCKS = 1024   # reduction grid (default)
FIN_G = 128            # finalize: partial groups merged in parallel
FUSE_MAX_G = 160       # finalize + apply in one launch up to this many partials
FUSE_C = 64            # ... per 64-channel chunk
FUSE_Q = 16            # ... 16 lanes a channel
FUSE_ROWS = 128        # rows per pass of the fused apply's 1024 threads
SMALL_MAX_M = 768      # one-launch kernels: 3 rows x 256 (forward), 6 x 128 (backward)


def _cdiv(a: int, b: int) -> int:
    return -(-a // b)


def plain_kind(M: int, C: int, fuse: bool = True) -> int:
    """0: reduce / finalize / apply, 1: reduce + fused finalize-apply, 2: one launch."""
    if not fuse or C % FUSE_C:
        return 0
    return 2 if M <= SMALL_MAX_M else 1


def make_plan(M: int, C: int, fuse: bool = True, tuning=(0, 0)) -> dict:
    tb = tuning[0] if tuning[0] > 0 else TARGET_BLOCKS
    un = 8 if tuning[1] == 8 else UNROLL
    chunk = min(C, MAX_CHUNK)
    nchunks = _cdiv(C, chunk)
    tpr = chunk // 8
    rpb = THREADS // tpr
    kind = plain_kind(M, C, fuse)
    target = max((128 if kind == 1 else tb) // nchunks, 1)
    iters = _cdiv(_cdiv(M, rpb * target), un) * un
    rows = rpb * iters
    G = _cdiv(M, rows)
    return dict(kind=kind, chunk=chunk, nchunks=nchunks, rpb=rpb, dead=THREADS - rpb * tpr, rows_per_block=rows,
                G=G, unroll=un, steps=iters // un, last_chunk=C - (nchunks - 1) * chunk,
                last_rows=M - (G - 1) * rows)


def workspace(M: int, C: int, fuse: bool = True, tuning=(0, 0)) -> int:
    """fp32 elements, as vgpu_bn_workspace."""
    return 2 * make_plan(M, C, fuse, tuning)["G"] * C + 4 * C


def fused_grid(M: int, C: int) -> tuple[int, int, int]:
    """(chunks, row ranges R, rows per range) of bn_*_fused_kernel."""
    chunks = C // FUSE_C
    R = max(min(_cdiv(256, chunks), _cdiv(M, FUSE_ROWS)), 1)
    rows_per = _cdiv(M, R)
    return chunks, _cdiv(M, rows_per), rows_per


def fused_ok(G: int, C: int, fuse: bool = True) -> bool:
    return fuse and G <= FUSE_MAX_G and C % FUSE_C == 0


def edge_rows(M: int, C: int, fuse: bool = True, tuning=(0, 0), backward: bool = False) -> list[int]:
    """The rows where a plan changes hands: first and last, each side of a
    thread's row stride in the one-launch kernels (255/256/257, 511/512, 767;
    the backward's stride is 128), of a reduction block, of one unrolled step,
    and of a fused apply's row range."""
    p = make_plan(M, C, fuse, tuning)
    rows = {1, M - 1}
    if p["kind"] == 2:
        st = 128 if backward else 256
        for k in range(1, SMALL_MAX_M // st):
            rows |= {k * st - 1, k * st, k * st + 1}
        rows.add(767)
    else:
        rb, step = p["rows_per_block"], p["rpb"] * p["unroll"]
        rows |= {step - 1, step, rb - 1, rb, (p["G"] - 1) * rb - 1, (p["G"] - 1) * rb}
        if p["kind"] == 1:
            rp = fused_grid(M, C)[2]
            rows |= {rp - 1, rp}
    return sorted(r for r in rows if 0 < r < M)


# ---- fp32 / bf16 bit helpers ----------------------------------------------------------
def ordered(t: torch.Tensor) -> torch.Tensor:
    """fp32 -> int64 that counts representable values (adjacent floats differ by 1)."""
    i = t.contiguous().view(torch.int32).to(I64)
    return torch.where(i < 0, -(i & 0x7FFFFFFF), i)


def ulps(a: torch.Tensor, b: torch.Tensor) -> torch.Tensor:
    """|a - b| in fp32 steps; a NaN or inf counts as 2**40."""
    a, b = a.detach().cpu().float(), b.detach().cpu().float()
    d = (ordered(a) - ordered(b)).abs()
    return torch.where(torch.isfinite(a) & torch.isfinite(b), d, torch.full_like(d, 1 << 40))


def bf16_choices(ref32: torch.Tensor) -> torch.Tensor:
    """[3, ...] bf16: the fp32 reference and its two fp32 neighbours, each rounded
    once.  They differ only where the reference is within 1 ulp of a tie."""
    up = torch.nextafter(ref32, torch.full_like(ref32, float("inf")))
    dn = torch.nextafter(ref32, torch.full_like(ref32, float("-inf")))
    return torch.stack([ref32.to(BF), up.to(BF), dn.to(BF)])


def act_ref(z: torch.Tensor, act: str) -> torch.Tensor:
    return z.clamp(min=0) if act == "relu" else z.clamp(0, 6) if act == "relu6" else z


def act_mask(z: torch.Tensor, act: str) -> torch.Tensor:
    """d act / dz as the kernels define it: relu z > 0, relu6 0 < z < 6."""
    if act == "relu":
        return (z > 0).to(z.dtype)
    if act == "relu6":
        return ((z > 0) & (z < 6)).to(z.dtype)
    return torch.ones_like(z)


# ---- Part A: forward inputs and statistics --------------------------------------------
OFFSETS = (0, 3, -5, 17, -40, 100, -200, 200, 64, -128, 1)   # 11 values: every 8-channel vector mixes them
GAMMAS = (0.5, 0.75, 1.0, 1.25, 1.5, 2.0, -1.0, 0.875, 1.0)  # bf16-exact
BETAS = (0.0, 0.5, -0.25, 1.0, 2.0, -1.0, 3.0, 0.125, 0.0, -2.0, 1.5, 0.25, 4.0)
EPS = float(torch.tensor(1e-5, dtype=F32))                   # the fp32 the kernel is given, as a double


def offsets(C: int) -> torch.Tensor:
    return torch.tensor([OFFSETS[c % len(OFFSETS)] for c in range(C)], dtype=I64)


def const_channel(C: int) -> int:
    return C // 2 + 1


def fwd_params(C: int):
    """(gamma, beta, old running mean, old running var) fp64, each exact in bf16.
    The old mean is a multiple of 4 near the channel's offset: 0.75 * old is an
    integer and 0.75 * old + 0.25 * mean lands in the mean's own binade."""
    c = torch.arange(C)
    gamma = torch.tensor(GAMMAS, dtype=F64)[(c * 2) % len(GAMMAS)]
    beta = torch.tensor(BETAS, dtype=F64)[(c * 5) % len(BETAS)]
    rm = (torch.round(offsets(C).double() / 4) * 4)
    rv = torch.full((C,), 3.0, dtype=F64)
    return gamma, beta, rm, rv


def fwd_input(M: int, C: int, mode: str, rstar: int = 0, seed: int = 0) -> torch.Tensor:
    """int64 [M, C].  Row 0 holds offset -+ 8 (a sign per channel); `dense`: every
    other row lies 8..16 away from it on the other side; `single`: every row
    equals row 0 except rstar.  Channel const_channel(C) is constant."""
    g = gen(seed * 7919 + M * 31 + C)
    sg = signs((C,), g)
    off = offsets(C)
    d0 = -8 * sg
    if mode == "dense":
        d = sg * torch.randint(0, 9, (M, C), generator=g)
        d[0] = d0
    else:
        assert mode == "single" and 0 < rstar < M
        d = d0.expand(M, C).clone()
        d[rstar] = sg * torch.randint(0, 9, (C,), generator=g)
    d[:, const_channel(C)] = d0[const_channel(C)]
    return off + d


@dataclasses.dataclass
class Stats:
    M: int
    S1: torch.Tensor        # int64: sum of x - x0
    S2: torch.Tensor        # int64: sum of (x - x0)**2
    mean: torch.Tensor      # fp64
    var: torch.Tensor       # fp64, biased
    invstd: torch.Tensor    # fp64
    unbiased: torch.Tensor  # fp64
    mean_exact: torch.Tensor  # bool: the mean is an integer (S1 % M == 0)


def stats_from_sums(x0: torch.Tensor, S1: torch.Tensor, S2: torch.Tensor, M: int, eps: float = EPS) -> Stats:
    """int64 sums -> fp64 statistics: one division each, then 1 / sqrt.  The
    numerator M * S2 - S1**2 is an exact int64 (below 2**53)."""
    num = M * S2 - S1 * S1
    assert int(num.min()) >= 0 and int(num.max()) < 2 ** 53
    var = num.double() / float(M * M)
    mean = x0.double() + S1.double() / M
    return Stats(M, S1, S2, mean, var, 1.0 / torch.sqrt(var + eps), var * M / (M - 1) if M > 1 else var,
                 S1 % M == 0)


def fwd_stats(x: torch.Tensor, eps: float = EPS) -> Stats:
    e = x - x[0]
    return stats_from_sums(x[0], e.sum(0), (e * e).sum(0), x.shape[0], eps)


def fwd_ref(x: torch.Tensor, st: Stats, gamma, beta, act: str, add=None):
    """(z, delta) fp64 [M, C]: z = act(x * s + t) (+ add) from the exact
    statistics; delta = 8 * 2**-24 * (|x s| + |mean s| + |beta|), eight fp32
    half-ulps of the terms the kernel rounds."""
    C = x.shape[1]
    gamma = torch.ones(C, dtype=F64) if gamma is None else gamma
    beta = torch.zeros(C, dtype=F64) if beta is None else beta
    s = gamma * st.invstd
    t = beta - st.mean * s
    xs = x.double() * s
    z = act_ref(xs + t, act)
    if add is not None:
        z = z + add.double()
    delta = 8 * 2.0 ** -24 * (xs.abs() + (st.mean * s).abs() + beta.abs())
    return z, delta


def y_bound(z: torch.Tensor, delta: torch.Tensor) -> torch.Tensor:
    """bf16's half-ulp of z plus 2 * delta."""
    return 2.0 ** -8 * z.abs() + 2 * delta


def row_sensitivity(x: torch.Tensor, st: Stats, eps: float = EPS):
    """fp32 ulps [M, C] by which the saved mean / invstd move when row r is lost
    (the same as counted twice, with the sign turned): the larger of the two."""
    e = x - x[0]
    out = None
    for sign in (-1, 1):
        S1 = st.S1 + sign * e
        S2 = st.S2 + sign * e * e
        mean = x[0].double() + S1.double() / st.M
        var = ((st.M * S2 - S1 * S1).double() / float(st.M * st.M)).clamp(min=0)
        inv = 1.0 / torch.sqrt(var + eps)
        moved = torch.maximum(ulps(mean.float(), st.mean.float().expand_as(mean)),
                              ulps(inv.float(), st.invstd.float().expand_as(inv)))
        out = moved if out is None else torch.minimum(out, moved)
    return out


# ---- Part B: backward -----------------------------------------------------------------
# (invstd, gamma, beta): s = gamma * invstd is a power of two, beta an integer
BWD_COMBOS = ((1.0, 1.0, 0.0), (1.0, 1.0, -2.0), (1.0, -1.0, 2.0), (0.5, 2.0, 1.0), (0.5, 1.0, 2.0), (0.25, 2.0, 2.0),
              (1.0, 2.0, 0.0), (0.25, 1.0, 1.0), (1.0, 0.5, 3.0), (0.25, -4.0, 0.0), (0.5, 1.0, -1.0))


@dataclasses.dataclass
class BwdCase:
    x: torch.Tensor        # int64 [M, C]
    dy: torch.Tensor       # int64 [M, C]
    add: torch.Tensor      # int64 [M, C]
    mean: torch.Tensor     # fp64 [C], integers
    invstd: torch.Tensor   # fp64 [C], 1, 1/2 or 1/4
    gamma: torch.Tensor    # fp64 [C] or None (affine=False: 1)
    beta: torch.Tensor     # fp64 [C] or None (0)
    z0: torch.Tensor       # bool [M, C]: planted z == 0
    z6: torch.Tensor       # bool [M, C]: planted z == 6


def bwd_case(M: int, C: int, mode: str, rstar: int = 0, affine: bool = True, seed: int = 0) -> BwdCase:
    """x = mean + d with integer mean (the channel's offset) and |d| <= 8; rows
    r % 7 == 0 hold the d that makes z exactly 0 and rows r % 7 == 3 the one that
    makes it 6, in every channel where that d is an integer within +-8.
    `dense`: dy in {-4..4} \\ {0} everywhere; `single`: dy is zero except in row
    rstar, where z = x s + t is moved strictly inside (0, 6)."""
    g = gen(seed * 104729 + M * 17 + C)
    k = (torch.arange(C) * 3) % len(BWD_COMBOS)
    combos = torch.tensor(BWD_COMBOS, dtype=F64)
    invstd = combos[k, 0]
    gamma, beta = (combos[k, 1], combos[k, 2]) if affine else (None, None)
    s = invstd * (gamma if affine else 1.0)
    b = beta if affine else torch.zeros(C, dtype=F64)
    mean = offsets(C).double()
    d = torch.randint(-8, 9, (M, C), generator=g)
    rows = torch.arange(M)
    z0 = torch.zeros((M, C), dtype=torch.bool)
    z6 = torch.zeros((M, C), dtype=torch.bool)
    for target, every, mask in ((0.0, 0, z0), (6.0, 3, z6)):
        dt = (target - b) / s
        ok = (dt == dt.round()) & (dt.abs() <= 8)
        at = (rows % 7 == every).view(-1, 1) & ok.view(1, -1)
        d = torch.where(at, dt.to(I64).expand(M, C), d)
        mask |= at
    if mode == "dense":
        dy = nonzero_ints((M, C), g, 4)
    else:
        assert mode == "single" and 0 < rstar < M
        grid = torch.arange(-8, 9).view(-1, 1)  # the first d in -8..8 with 0 < d s + b < 6
        inside = (grid.double() * s + b > 0) & (grid.double() * s + b < 6)
        assert bool(inside.any(0).all())
        d[rstar] = grid.expand(-1, C).gather(0, inside.int().argmax(0).view(1, C))[0]
        z0[rstar] = z6[rstar] = False
        dy = torch.zeros((M, C), dtype=I64)
        dy[rstar] = nonzero_ints((C,), g, 4)
    add = torch.randint(-8, 9, (M, C), generator=g)
    return BwdCase(offsets(C) + d, dy, add, mean, invstd, gamma, beta, z0, z6)


def bwd_ref(c: BwdCase, act: str, with_add: bool):
    """(dgamma fp64 [C] exact, dbeta fp64 [C] exact, dx fp64 [M, C], bound [M, C],
    terms: the largest sum of |dz x-hat| over a channel).  z, the mask, dz,
    x-hat and both sums are exact in fp64 (multiples of 1/8 far below 2**53)."""
    M, C = c.x.shape
    gamma = torch.ones(C, dtype=F64) if c.gamma is None else c.gamma
    beta = torch.zeros(C, dtype=F64) if c.beta is None else c.beta
    s = gamma * c.invstd
    x = c.x.double()
    z = (x - c.mean) * s + beta
    dz = c.dy.double() * act_mask(z, act)
    xhat = (x - c.mean) * c.invstd
    dbeta = dz.sum(0)
    dgamma = (dz * xhat).sum(0)
    dx, bound = dx_ref(x, dz, c.add if with_add else None, s, c.mean, c.invstd, dgamma, dbeta, M)
    return dgamma, dbeta, dx, bound, float((dz * xhat).abs().sum(0).max())


def dx_ref(x, dz, add, s, mean, invstd, dgamma, dbeta, M):
    """dx = s (dz - dbeta / M - x-hat dgamma / M) (+ add) in fp64, and the bound
    2**-8 |dx| + 2 * 8 * 2**-24 (|s dz| + |cc x| + |s dbeta / M| + |mean cc|)."""
    xhat = (x - mean) * invstd
    dx = s * (dz - dbeta / M - xhat * dgamma / M)
    if add is not None:
        dx = dx + add.double()
    cc = -s * invstd * dgamma / M
    bound = 2.0 ** -8 * dx.abs() + 2 * 8 * 2.0 ** -24 * (
        (s * dz).abs() + (cc * x).abs() + (s * dbeta / M).abs() + (mean * cc).abs())
    return dx, bound


# ---- Part B: the *_partials entry points ----------------------------------------------
def split_sum(total: torch.Tensor, G: int, g, spread: int = 1000) -> torch.Tensor:
    """int64 [C] -> int64 [G, C]: non-zero integers of either sign, total // G plus
    noise of up to +-spread each, that sum to total."""
    C = total.numel()
    if G == 1:
        assert bool((total != 0).all())
        return total.view(1, C).clone()
    parts = total // G + nonzero_ints((G, C), g, spread)
    parts[:G - 1] = torch.where(parts[:G - 1] == 0, 1, parts[:G - 1])
    parts[G - 1] = total - parts[:G - 1].sum(0)
    fix = parts[G - 1] == 0   # move a unit or two from the last group to the one before
    step = torch.where(parts[G - 2] == -1, 2, 1)
    parts[G - 1] = torch.where(fix, -step, parts[G - 1])
    parts[G - 2] = torch.where(fix, parts[G - 2] + step, parts[G - 2])
    assert bool((parts != 0).all()) and torch.equal(parts.sum(0), total)
    return parts


@functools.lru_cache(maxsize=4)
def fwd_partials_case(M: int, C: int, seed: int = 0):
    """Integer mean (non-zero) and var in {1, 4, 16} per channel; S1 = M mean
    and S2 = M (var + mean**2) split into G = ceil(M / 64) pairs; x = mean + d,
    |d| <= 8; gamma a power of two, beta an integer.  With eps = 0 mean, invstd,
    s, t and y are exact.  -> dict of tensors (partial fp32 [G, C, 2])."""
    G = _cdiv(M, 64)
    g = gen(seed * 15485863 + M * 13 + C)
    c = torch.arange(C)
    mean = offsets(C)
    mean = torch.where(mean == 0, 7, mean)
    var = torch.tensor((1, 4, 16), dtype=I64)[(c * 2 + c // 8) % 3]
    p1 = split_sum(M * mean, G, g)
    p2 = split_sum(M * (var + mean * mean), G, g, 100000)
    partial = torch.stack([p1, p2], -1)
    gamma = torch.tensor((1.0, 2.0, -1.0, 0.5, 1.0, -2.0, 0.5), dtype=F64)[c % 7]
    beta = torch.tensor((0.0, 1.0, -2.0, 3.0, 2.0, -1.0), dtype=F64)[c % 6]
    invstd = 1.0 / torch.sqrt(var.double())
    s = gamma * invstd
    d = torch.randint(-8, 9, (M, C), generator=g)
    rows = torch.arange(M)
    for target, every in ((0.0, 0), (6.0, 3)):
        dt = (target - beta) / s
        ok = (dt == dt.round()) & (dt.abs() <= 8)
        d = torch.where((rows % 7 == every).view(-1, 1) & ok.view(1, -1), dt.to(I64).expand(M, C), d)
    x = mean + d
    z = d.double() * s + beta
    rm_old = torch.round(mean.double() / 4) * 4
    return dict(G=G, partial=partial, mean=mean.double(), var=var.double(), invstd=invstd, gamma=gamma, beta=beta,
                s=s, t=beta - mean.double() * s, x=x, z=z, rm_old=rm_old, rv_old=torch.full((C,), 3.0, dtype=F64),
                unbiased=var.double() * M / (M - 1) if M > 1 else var.double())


@functools.lru_cache(maxsize=4)
def bwd_partials_case(M: int, C: int, seed: int = 0):
    """Synthetic integer pairs (sum dz, sum dz x-hat) of G = ceil(M / 64) groups,
    chosen mean / invstd / gamma / beta as bwd_case, integer dz (|dz| <= 4), x
    and add.  The sums are NOT those of dz: the entry point takes them as given."""
    G = _cdiv(M, 64)
    g = gen(seed * 32452843 + M * 11 + C)
    base = bwd_case(M, C, "dense", seed=seed + 1)
    tot1 = torch.randint(-3000, 3001, (C,), generator=g)
    tot2 = torch.randint(-3000, 3001, (C,), generator=g)
    tot1 = torch.where(tot1 == 0, 5, tot1)
    tot2 = torch.where(tot2 == 0, -5, tot2)
    partial = torch.stack([split_sum(tot1, G, g, 64), split_sum(tot2, G, g, 64)], -1)
    return dict(G=G, partial=partial, dbeta=tot1.double(), dgamma=tot2.double(), case=base)


# ---- Part C: statistics from the convolution's epilogue -------------------------------
# n, c, h, w, cout, ks, stride, pad, residual.  M = n * oh * ow is no multiple
# of 64 and every image straddles a 64-row group.
CONV_KINDS = {
    "1x1": (2, 128, 9, 11, 64, 1, 1, 0, False),       # M = 198
    "1x1_res": (2, 128, 9, 11, 128, 1, 1, 0, True),
    "3x3": (3, 128, 7, 5, 128, 3, 1, 1, False),       # M = 105; Cout % 128 == 0 and no residual: the halo kernel's
    "3x3_res": (3, 128, 7, 5, 64, 3, 1, 1, True),
    "3x3_s2": (3, 64, 13, 11, 64, 3, 2, 1, False),    # M = 3 * 7 * 6 = 126
}
CONV_MODES = ("tile64", "tile128", "halo128", "halo256")


def conv_modes(kind: str):
    return CONV_MODES if kind == "3x3" else CONV_MODES[:2]


@functools.lru_cache(maxsize=8)
def conv_case(kind: str):
    """x int64 [N, H, W, C] in {-2..2} \\ {0}; W int64 [Cout, KS, KS, C] with one +-1
    per reduction index in a pseudo-random output channel (as _exact.splitk_case);
    residual int64 [M, Cout] in {-4..4} or None; y int64 [M, Cout], the
    convolution alone; and a BatchNorm over Cout (bwd_case: integer mean, invstd
    and s powers of two, x-hat planted at z == 0 and z == 6) for the backward."""
    n, c, h, w, cout, ks, s, p, has_res = CONV_KINDS[kind]
    g = gen(len(kind) * 101 + c + cout)
    x = nonzero_ints((n, h, w, c), g)
    K = ks * ks * c
    wt = torch.zeros((cout, K), dtype=I64)
    co = torch.randint(0, cout, (K,), generator=g)
    co[torch.randperm(K, generator=g)[:cout]] = torch.arange(cout)  # every output channel has a term
    wt[co, torch.arange(K)] = signs((K,), g)
    wt = wt.view(cout, ks, ks, c)
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), wt.permute(0, 3, 1, 2).double(), stride=s, padding=p)
    y = y.round().to(I64).permute(0, 2, 3, 1)
    oh, ow = y.shape[1:3]
    M = n * oh * ow
    res = torch.randint(-4, 5, (M, cout), generator=g) if has_res else None
    return dict(x=x, w=wt, res=res, y=y.reshape(M, cout), M=M, G=_cdiv(M, 64), oh=oh, ow=ow,
                bn=bwd_case(M, cout, "dense", seed=7))


def group_sums(v: torch.Tensor, q: torch.Tensor) -> torch.Tensor:
    """fp64 [G, C, 2]: (sum v, sum v q) over each group of 64 rows of [M, C]."""
    M, C = v.shape
    G = _cdiv(M, 64)
    z = torch.zeros((G * 64 - M, C), dtype=F64)
    v, q = torch.cat([v.double(), z]), torch.cat([q.double(), z])
    return torch.stack([v.view(G, 64, C).sum(1), (v * q).view(G, 64, C).sum(1)], -1)


def conv_fwd_ref(case):
    """(stored y int64 [M, Cout], statistics fp64 [G, Cout, 2] = (sum y, sum y**2))."""
    y = case["y"] if case["res"] is None else case["y"] + case["res"]
    return y, group_sums(y, y)


def conv_bwd_ref(case, act: str):
    """With the conv's output taken as the gradient of the BatchNorm's output:
    (stored dy * act'(z) fp64 [M, Cout], statistics (sum, sum * x-hat), coef fp64 [4, Cout])."""
    bn = case["bn"]
    s = bn.gamma * bn.invstd
    t = bn.beta - bn.mean * s
    x = bn.x.double()
    v = (case["y"] if case["res"] is None else case["y"] + case["res"]).double() * act_mask(x * s + t, act)
    return v, group_sums(v, (x - bn.mean) * bn.invstd), torch.stack([s, t, bn.mean, bn.invstd])


# ---- the case lists -------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Plain:
    """A plain-path shape and the switches it runs under.  fuse: -1 default, 0 off."""
    M: int
    C: int
    what: str
    fuse: int = -1
    tuning: tuple = (0, 0)
    act: str = "relu"
    bf16: bool = False
    entry: str = "train"      # train | coef | add
    affine: bool = True
    running: bool = True
    single: bool = False      # also run with every row equal to row 0 but one, at each of edge_rows

    @property
    def plan(self) -> dict:
        return make_plan(self.M, self.C, self.fuse != 0, self.tuning)

    @property
    def id(self) -> str:
        t = "" if self.tuning == (0, 0) else "-t%dx%d" % self.tuning
        return f"{self.M}x{self.C}{'-nofuse' if self.fuse == 0 else ''}{t}-{self.act}" \
               f"-{'bf16' if self.bf16 else 'fp32'}-{self.entry}{'' if self.affine else '-noaffine'}{'' if self.running else '-norunning'}"


PLAIN = [
    # kind 2: one launch (C % 64 == 0, M <= 768)
    Plain(2, 64, "one launch, two rows", act="none"),
    Plain(255, 64, "one launch, first row slot one short", act="relu6", bf16=True),
    Plain(256, 64, "one launch, first row slot full", entry="coef"),
    Plain(257, 64, "one launch, one row in the second slot", act="relu6", entry="add"),
    Plain(513, 64, "one launch, one row in the third slot", bf16=True, entry="coef", affine=False),
    Plain(767, 64, "one launch, one row short of full", act="none", running=False),
    Plain(768, 64, "one launch, full", act="relu6", single=True),
    Plain(257, 960, "one launch, 30 workgroups", bf16=True, entry="add", single=True),
    Plain(768, 960, "one launch, 30 workgroups, full", act="none", entry="coef"),
    # kind 1: reduce + fused finalize / apply
    Plain(769, 64, "fused, first size past the one-launch limit", act="relu6", single=True),
    Plain(1000, 64, "fused", bf16=True, entry="add", act="none"),
    Plain(4097, 64, "fused, 32 row ranges and one row", entry="coef", act="relu6"),
    Plain(769, 192, "fused, 3 chunks", act="none", affine=False, bf16=True),
    Plain(1000, 192, "fused, 3 chunks", entry="add"),
    Plain(4097, 192, "fused, 3 chunks", bf16=True, running=False, act="relu6", single=True),
    Plain(769, 1024, "fused, two reduction chunks, 16 fused chunks", entry="coef", single=True),
    Plain(1000, 1024, "fused, two reduction chunks, 16 fused chunks", act="relu6", bf16=True),
    # kind 0: reduce / finalize / apply
    Plain(5, 96, "three launches, G = 1, 21 rows per block pass, 4 dead threads", act="none"),
    Plain(1, 96, "three launches, one row"),
    Plain(1, 64, "one launch, one row", act="none", bf16=True),
    Plain(1000, 96, "three launches, partial last block", act="relu6", bf16=True, single=True),
    Plain(10837, 96, "three launches, G = 130 > 128, one row in the last block", entry="coef", single=True),
    Plain(3001, 8, "three launches, one thread per row", act="relu6", single=True),
    Plain(1030, 8, "three launches, one thread per row, partial last block", bf16=True, affine=False, act="none"),
    Plain(1000, 520, "three launches, second chunk of 8 channels", act="relu6", entry="coef", single=True),
    Plain(777, 1000, "three launches, second chunk of 488 channels", bf16=True, single=True),
    Plain(300, 64, "three launches, fuse off (else one launch)", fuse=0, act="relu6"),
    Plain(1000, 64, "three launches, fuse off (else fused)", fuse=0, bf16=True, running=False, single=True),
    Plain(3001, 96, "target 2 blocks, unroll 8: 9 steps of 168 rows", tuning=(2, 8), act="relu6", single=True),
    Plain(3001, 192, "target 8 blocks, unroll 4: 10 steps of 40 rows, fuse off", fuse=0, tuning=(8, 4), bf16=True,
          entry="coef", single=True),
    Plain(2999, 64, "fused plan with unroll 8", tuning=(2, 8), act="none", single=True),
]
# shapes on which the add entry must answer -2 (three launches)
NO_ADD = [Plain(1000, 96, "no add form: C % 64"), Plain(300, 64, "no add form: fuse off", fuse=0)]
SINGLE = [p for p in PLAIN if p.single]

PARTIALS_G = (1, 2, 127, 128, 129, 160, 161, 300)


def _partials_m(G: int, i: int) -> int:
    """Rows for G groups with M % 64 cycling through 0, 1, 63."""
    return (64 * G, 64 * (G - 1) + 1, 64 * (G - 1) + 63)[i % 3]


@dataclasses.dataclass(frozen=True)
class Part:
    M: int
    C: int
    act: str = "relu"
    bf16: bool = False
    running: bool = True
    fuse: int = -1

    @property
    def G(self) -> int:
        return _cdiv(self.M, 64)

    @property
    def fused(self) -> bool:
        return fused_ok(self.G, self.C, self.fuse != 0)

    @property
    def id(self) -> str:
        return f"G{self.G}-{self.M}x{self.C}-{self.act}-{'bf16' if self.bf16 else 'fp32'}" \
               f"{'' if self.running else '-norunning'}{'-nofuse' if self.fuse == 0 else ''}"


_ACTS = ("none", "relu", "relu6")
PARTIALS = [Part(_partials_m(G, i + j), C, _ACTS[(i + j) % 3], bool((i + j) % 2), running=(i + 2 * j) % 4 != 3)
            for i, G in enumerate(PARTIALS_G) for j, C in enumerate((64, 96))] + \
           [Part(64 * 160, 64, "relu6", True), Part(64 * 160 + 1, 64, "relu6", True),
            Part(64 * 2 + 1, 64, "none", False, fuse=0), Part(63, 128, "relu", True)]


def assert_bn_coverage(plain=PLAIN, single=SINGLE, partials=PARTIALS, no_add=NO_ADD) -> None:
    """The lists reach every plan, branch and entry point named in the module docstrings."""
    plans = [(p, p.plan) for p in plain]

    def has(pred):
        return any(pred(p, pl) for p, pl in plans)

    k2 = {(p.M, p.C) for p, pl in plans if pl["kind"] == 2}
    assert {(m, 64) for m in (2, 255, 256, 257, 513, 767, 768)} <= k2 and any(c == 960 for _, c in k2)
    k1 = {(p.M, p.C) for p, pl in plans if pl["kind"] == 1}
    assert {m for m, _ in k1} >= {769, 1000, 4097} and {c for _, c in k1} >= {64, 192, 1024}
    assert has(lambda p, pl: pl["kind"] == 1 and pl["nchunks"] == 2 and fused_grid(p.M, p.C)[0] == 16)
    assert has(lambda p, pl: pl["kind"] == 1 and fused_grid(p.M, p.C)[2] % FUSE_ROWS != 0)
    assert has(lambda p, pl: pl["kind"] == 1 and fused_grid(p.M, p.C)[1] > 1)
    # a fused apply with one row range: only the partials entry points reach it (the plain path has M > 768)
    assert any(q.fused and fused_grid(q.M, q.C)[1] == 1 for q in partials)
    assert all(pl["G"] <= 128 for p, pl in plans if pl["kind"] == 1)
    k0 = [(p, pl) for p, pl in plans if pl["kind"] == 0]
    assert any(p.C == 96 and pl["rpb"] == 21 and pl["dead"] == 4 for p, pl in k0)
    assert any(p.C == 8 and pl["rpb"] == 256 for p, pl in k0)
    assert {pl["last_chunk"] for p, pl in k0 if pl["nchunks"] == 2} >= {8, 488}
    assert any(p.C == 64 and p.fuse == 0 for p, pl in k0)
    assert any(pl["G"] > 1 and pl["last_rows"] < pl["rows_per_block"] for p, pl in k0)
    assert any(pl["G"] == 1 for p, pl in k0) and any(pl["G"] > FIN_G for p, pl in k0)
    assert any(p.tuning == (2, 8) and pl["unroll"] == 8 and pl["steps"] >= 8 and 2900 < p.M < 3100 for p, pl in k0)
    assert any(p.tuning == (8, 4) and pl["unroll"] == 4 and pl["steps"] >= 8 and 2900 < p.M < 3100 for p, pl in k0)
    assert any(p.M == 1 for p in plain)
    for kind in (0, 1, 2):
        mine = [p for p, pl in plans if pl["kind"] == kind]
        assert {p.act for p in mine} == set(ACT) and {p.bf16 for p in mine} == {False, True}, kind
        assert any(not p.affine for p in mine) and any(not p.running for p in mine), kind
        assert any(p.entry == "coef" for p in mine), kind
        assert any(pl["kind"] == kind for pl in (s.plan for s in single)), kind
    assert any(p.entry == "add" and pl["kind"] == 1 for p, pl in plans)
    assert any(p.entry == "add" and pl["kind"] == 2 for p, pl in plans)
    assert no_add and all(p.plan["kind"] == 0 for p in no_add)
    # partials
    for C in (64, 96):
        assert {q.G for q in partials if q.C == C} >= set(PARTIALS_G), C
    assert any(q.C == 64 and q.G == 160 and q.fused for q in partials)
    assert any(q.C == 64 and q.G == 161 and not q.fused for q in partials)
    assert not any(q.fused for q in partials if q.C == 96)
    assert {q.M % 64 for q in partials} >= {0, 1, 63}
    assert any(not q.fused and q.G > FIN_G for q in partials) and any(not q.fused and q.G < FIN_G for q in partials)
    for fused in (False, True):
        mine = [q for q in partials if q.fused == fused]
        assert {q.act for q in mine} == set(ACT) and {q.bf16 for q in mine} == {False, True}
        assert any(not q.running for q in mine)
    assert max(p.M * p.C for p in plain) <= 1100000 and max(q.M * q.C for q in partials) <= 1900000
    assert FP32_EXACT > 256 * max(p.M for p in plain)
