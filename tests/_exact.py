"""Exact-integer inputs and int64 references for the kernels whose reduction is
long or split across workgroups (conv_wgrad.hip, skinny.hip, dwconv.hip and the
forward split-K of conv_gemm.hip).  Pure CPU torch.

With small-integer bf16 operands every product and every fp32 partial sum is an
integer below 2**24, exact in any summation order, so a kernel must reproduce
the reference bit for bit.  Two conditions make that comparison see a single
lost term; tests/test_exact_cpu.py asserts both on the REFERENCE of every case:

1. representability: a bf16 output has max|ref| <= 128 (all integers up to 256
   are exact in bf16, so a wrong integer either differs or rounds to >= 256);
   an fp32 output has max|ref| < 2**24;
2. visibility: every index of the reduction contributes a non-zero term to at
   least one output element.

Long reductions get there with one-hot operands: at each reduction index each
operand is non-zero in one pseudo-randomly chosen channel, with value +-1.
"""
from __future__ import annotations

import functools

import torch

BF16_EXACT = 128          # condition 1 for bf16 outputs
FP32_EXACT = 2 ** 24      # condition 1 for fp32 outputs and partials
CL = torch.channels_last
I64 = torch.int64


def gen(seed: int) -> torch.Generator:
    return torch.Generator(device="cpu").manual_seed(seed)


def signs(shape, g) -> torch.Tensor:
    """+-1, int64."""
    return torch.randint(0, 2, shape, generator=g, dtype=I64) * 2 - 1


def nonzero_ints(shape, g, hi: int = 2) -> torch.Tensor:
    """Uniform over {-hi..-1, 1..hi}, int64."""
    return torch.randint(1, hi + 1, shape, generator=g, dtype=I64) * signs(shape, g)


def out_hw(h: int, w: int, ks: int, stride: int, pad: int) -> tuple[int, int]:
    return (h + 2 * pad - ks) // stride + 1, (w + 2 * pad - ks) // stride + 1


def to_nchw_cl(t_nhwc: torch.Tensor) -> torch.Tensor:
    """Integer [N,H,W,C] -> bf16 [N,C,H,W] in channels_last memory."""
    return t_nhwc.permute(0, 3, 1, 2).to(torch.bfloat16).contiguous(memory_format=CL)


def round_to(ref: torch.Tensor, dtype: torch.dtype) -> torch.Tensor:
    """The integer reference rounded once to the kernel's output type."""
    return ref.to(torch.float64).to(dtype)


# ---- convolution weight gradient ------------------------------------------------------
# dW[co][kh][kw][c] = sum_{n,oh,ow} dy[n][oh][ow][co] * x[n][oh*s-p+kh][ow*s-p+kw][c]

class WgradCase:
    """x [N,C,H,W] / dy [N,Cout,OH,OW] bf16 channels_last and ref int64 [Cout,KS,KS,C]."""

    def __init__(self, shape, mode, x_nhwc, dy_nhwc, ref):
        self.shape, self.mode = shape, mode
        self.x_nhwc, self.dy_nhwc, self.ref = x_nhwc, dy_nhwc, ref

    @property
    def x(self):
        return to_nchw_cl(self.x_nhwc)

    @property
    def dy(self):
        return to_nchw_cl(self.dy_nhwc)

    def ref_as_weight(self) -> torch.Tensor:
        """bf16 [Cout,C,KS,KS] (channels_last values), as conv2d_wgrad returns it."""
        return round_to(self.ref, torch.bfloat16).permute(0, 3, 1, 2)


def _onehot(idx: torch.Tensor, sgn: torch.Tensor, c: int) -> torch.Tensor:
    """[..] channel index and sign -> int8 [.., c] with one non-zero per position."""
    out = torch.zeros((*idx.shape, c), dtype=torch.int8)
    out.scatter_(-1, idx.unsqueeze(-1), sgn.to(torch.int8).unsqueeze(-1))
    return out


def wgrad_onehot(shape, seed: int = 0) -> WgradCase:
    """One-hot x and dy; the reference is one index_add_ per tap."""
    n, h, w, c, cout, ks, s, p = shape
    oh, ow = out_hw(h, w, ks, s, p)
    g = gen(seed)
    fx = torch.randint(0, c, (n, h, w), generator=g)
    sx = signs((n, h, w), g)
    fd = torch.randint(0, cout, (n, oh, ow), generator=g)
    sd = signs((n, oh, ow), g)
    ref = torch.zeros(cout * ks * ks * c, dtype=I64)
    ohs = torch.arange(oh).view(1, oh, 1).expand(n, oh, ow)
    ows = torch.arange(ow).view(1, 1, ow).expand(n, oh, ow)
    ns = torch.arange(n).view(n, 1, 1).expand(n, oh, ow)
    for kh in range(ks):
        for kw in range(ks):
            ih, iw = ohs * s - p + kh, ows * s - p + kw
            ok = (ih >= 0) & (ih < h) & (iw >= 0) & (iw < w)
            nn, ii, jj = ns[ok], ih[ok], iw[ok]
            at = ((fd[ok] * ks + kh) * ks + kw) * c + fx[nn, ii, jj]
            ref.index_add_(0, at, sd[ok] * sx[nn, ii, jj])
    return WgradCase(shape, "onehot", _onehot(fx, sx, c), _onehot(fd, sd, cout), ref.view(cout, ks, ks, c))


DENSE_PIXELS = 32  # dense values of magnitude <= 2 at <= 32 pixels: |ref| <= 32 * 4 = 128


def wgrad_dense(shape, seed: int = 0) -> WgradCase:
    """The dense companion: x in {-2..2} \\ {0} everywhere, dy in {-2..2} \\ {0}
    on at most 32 output pixels spread over the whole pixel range (first and
    last included) and zero elsewhere, so every output element is a sum of up
    to 32 products and almost none is zero."""
    n, h, w, c, cout, ks, s, p = shape
    oh, ow = out_hw(h, w, ks, s, p)
    g = gen(seed + 1000)
    x = nonzero_ints((n, h, w, c), g).to(torch.int8)
    P = n * oh * ow
    m = min(P, DENSE_PIXELS)
    pix = torch.unique(torch.linspace(0, P - 1, m).round().to(I64))
    dyv = nonzero_ints((pix.numel(), cout), g)
    dy = torch.zeros((P, cout), dtype=torch.int8)
    dy[pix] = dyv.to(torch.int8)
    ref = torch.zeros((cout, ks, ks, c), dtype=I64)
    for j, q in enumerate(pix.tolist()):
        ni, r = divmod(q, oh * ow)
        oi, oj = divmod(r, ow)
        for kh in range(ks):
            for kw in range(ks):
                ih, iw = oi * s - p + kh, oj * s - p + kw
                if 0 <= ih < h and 0 <= iw < w:
                    ref[:, kh, kw, :] += torch.outer(dyv[j], x[ni, ih, iw].to(I64))
    return WgradCase(shape, "dense", x, dy.view(n, oh, ow, cout), ref)


@functools.lru_cache(maxsize=4)
def wgrad_case(shape, mode: str) -> WgradCase:
    return wgrad_onehot(shape) if mode == "onehot" else wgrad_dense(shape)


def wgrad_dense_ref(x_nhwc, dy_nhwc, ks, s, p) -> torch.Tensor:
    """torch.nn.grad.conv2d_weight in fp64 -> int64 [Cout,KS,KS,C] (small cases)."""
    x = x_nhwc.permute(0, 3, 1, 2).double()
    dy = dy_nhwc.permute(0, 3, 1, 2).double()
    cout, c = dy.shape[1], x.shape[1]
    r = torch.nn.grad.conv2d_weight(x, (cout, c, ks, ks), dy, stride=s, padding=p)
    return r.permute(0, 2, 3, 1).round().to(I64)


def wgrad_visible(case: WgradCase) -> bool:
    """Condition 2: at every output pixel dy is non-zero, and x is non-zero at
    one or more of the input pixels its taps read."""
    n, h, w, c, cout, ks, s, p = case.shape
    oh, ow = out_hw(h, w, ks, s, p)
    if not bool((case.dy_nhwc != 0).any(-1).all()):
        return False
    xnz = (case.x_nhwc != 0).any(-1)
    seen = torch.zeros((n, oh, ow), dtype=torch.bool)
    ohs, ows = torch.arange(oh).view(oh, 1), torch.arange(ow).view(1, ow)
    for kh in range(ks):
        for kw in range(ks):
            ih, iw = (ohs * s - p + kh).expand(oh, ow), (ows * s - p + kw).expand(oh, ow)
            ok = (ih >= 0) & (ih < h) & (iw >= 0) & (iw < w)
            seen |= ok & xnz[:, ih.clamp(0, h - 1), iw.clamp(0, w - 1)]
    return bool(seen.all())


# How conv_wgrad.hip lays a split count out over a shape (wgrad_impl).  The
# count itself comes from the library: the GPU test reads it from
# vgpu_conv_wgrad_workspace and holds it against the one listed in WGRAD_CASES.
def wgrad_plan(shape, splits: int) -> dict:
    """What a split count means for a shape: kernel, tile, reduce variant, steps
    per split, steps of the last working split and the number of empty splits."""
    n, h, w, c, cout, ks, s, p = shape
    oh, ow = out_hw(h, w, ks, s, p)
    P = n * oh * ow
    fused = ks == 3 and p == 1 and s in (1, 2) and P >= 65536
    if fused:
        total = n * oh * ((ow + 31) // 32)
        tile = (64, 64)
    else:
        total = (P + 31) // 32
        tile = (128 if cout % 128 == 0 else 64, 128 if c % 128 == 0 else 64)
    steps = (total + splits - 1) // splits
    working = (total + steps - 1) // steps
    red = 0 if splits == 1 else 16 if splits >= 64 else 8 if splits >= 32 else 4 if splits >= 16 else \
        2 if splits >= 8 else 1
    return dict(kernel=("wgrad3<%d>" % s) if fused else "wgrad", tile=tile, reduce=red, steps=steps,
                last=total - (working - 1) * steps, empty=splits - working, total=total, pixels=P)


def assert_wgrad_coverage(plans: list[dict]) -> None:
    """The cases reach every tile on the direct-write path, every reduce
    instantiation, an empty trailing split on every tile, both tap-fused
    kernels, a one-step loop, a last split of one step and an even step count
    with a ragged last step."""
    tiles = {(64, 64), (64, 128), (128, 64), (128, 128)}
    assert {p["tile"] for p in plans if p["kernel"] == "wgrad" and p["reduce"] == 0} == tiles
    assert {p["reduce"] for p in plans} == {0, 1, 2, 4, 8, 16}
    assert {p["tile"] for p in plans if p["kernel"] == "wgrad" and p["empty"] > 0} == tiles
    assert {p["kernel"] for p in plans} == {"wgrad", "wgrad3<1>", "wgrad3<2>"}
    assert any(p["kernel"].startswith("wgrad3") and p["empty"] > 0 for p in plans)
    assert any(p["kernel"].startswith("wgrad3") and p["empty"] == 0 and p["last"] < p["steps"] for p in plans)
    assert any(p["steps"] == 1 for p in plans) and any(p["last"] == 1 and p["steps"] > 1 for p in plans)
    assert any(p["pixels"] % 32 == 31 and p["total"] % 2 == 0 for p in plans)


# (shape, splits the heuristic gives, what it is there for); shape = (N,H,W,C,Cout,KS,stride,pad)
WGRAD_CASES = [
    # direct write (one split): one step; two steps with a ragged 31-pixel last step
    ((1, 3, 5, 64, 64, 3, 1, 1), 1, "direct 64x64, one step"),
    ((1, 3, 5, 128, 64, 3, 1, 1), 1, "direct BM64xBN128, one step"),
    ((1, 3, 5, 64, 128, 3, 1, 1), 1, "direct BM128xBN64, one step"),
    ((1, 3, 5, 128, 128, 3, 1, 1), 1, "direct 128x128, one step"),
    ((1, 15, 17, 64, 64, 3, 1, 1), 1, "direct 64x64, ragged last step"),
    ((1, 15, 17, 128, 64, 3, 1, 1), 1, "direct BM64xBN128, ragged last step"),
    ((1, 15, 17, 64, 128, 3, 1, 1), 1, "direct BM128xBN64, ragged last step"),
    ((1, 15, 17, 128, 128, 3, 1, 1), 1, "direct 128x128, ragged last step"),
    ((1, 3, 5, 64, 64, 1, 2, 0), 1, "direct strided 1x1, one step"),
    # every reduce instantiation
    ((1, 19, 21, 64, 64, 3, 1, 1), 4, "reduce<1>, last split of 1 step"),
    ((1, 17, 19, 128, 128, 3, 1, 1), 2, "reduce<1>, 2 splits"),
    ((1, 29, 31, 64, 64, 3, 1, 1), 8, "reduce<2>"),
    ((1, 43, 45, 64, 64, 3, 1, 1), 16, "reduce<4>"),
    ((1, 63, 65, 64, 64, 3, 1, 1), 32, "reduce<8>"),
    ((1, 89, 91, 64, 64, 3, 1, 1), 64, "reduce<16>, last split of 2 steps"),
    # trailing splits with nothing to do, on every tile shape
    ((1, 107, 109, 128, 64, 3, 1, 1), 64, "empty splits, BM64xBN128"),
    ((1, 129, 131, 128, 128, 1, 2, 0), 32, "empty splits, 128x128, strided 1x1"),
    ((1, 107, 109, 64, 128, 3, 1, 1), 64, "empty splits, BM128xBN64"),
    ((1, 67, 69, 128, 128, 3, 1, 1), 32, "empty splits, 128x128"),
    ((1, 129, 131, 64, 64, 1, 2, 0), 32, "empty splits, 64x64, strided 1x1"),
    # the tap-fused 3x3 kernels (P >= 65536)
    ((1, 257, 259, 64, 64, 3, 1, 1), 256, "wgrad3<1>: last row segment 3 px, 24 empty splits"),
    ((1, 257, 259, 128, 192, 3, 1, 1), 32, "wgrad3<1>: 2x3 tiles, last split 50 of 73 steps"),
    ((1, 515, 513, 64, 64, 3, 2, 1), 256, "wgrad3<2>: last row segment 1 px"),
]
# Cases also run through the library with guard rows and a NaN-filled workspace
WGRAD_GUARDED = [sh for sh, _, what in WGRAD_CASES if what.startswith("empty")] + [
    (1, 19, 21, 64, 64, 3, 1, 1), (1, 3, 5, 64, 128, 3, 1, 1), (1, 257, 259, 64, 64, 3, 1, 1)]


def wgrad_modes(shape) -> list[str]:
    """Small pixel counts are dense outright; the others get the one-hot
    operands and the dense companion."""
    n, h, w, c, cout, ks, s, p = shape
    oh, ow = out_hw(h, w, ks, s, p)
    return ["dense"] if n * oh * ow <= DENSE_PIXELS else ["onehot", "dense"]


# ---- bias-gradient reduce (db_reduce_block) -------------------------------------------
DB_SLABS = (1, 16, 17, 63, 64, 65, 130)
DB_CHANNELS = (8, 24, 64)


def db_case(slabs: int, c: int, stride: int, bf16: bool, seed: int = 0):
    """(partials fp32 [slabs, c, stride], ref int64 [c]).  Only element 0 of each
    stride group is part of the sum; the rest holds a value that would break it.
    A bf16 result gets two +-1 per slab (condition 1), an fp32 one dense {-3..3} \\ {0}."""
    g = gen(seed + slabs * 131 + c)
    if bf16:
        v = torch.zeros((slabs, c), dtype=I64)
        rows = torch.arange(slabs)
        for j in range(2):
            v[rows, (rows * 5 + 3 * j + torch.randint(0, c, (1,), generator=g)) % c] = signs((slabs,), g)
    else:
        v = nonzero_ints((slabs, c), g, 3)
    part = torch.full((slabs, c, stride), 4097.5, dtype=torch.float32)
    part[:, :, 0] = v.float()
    return part, v.sum(0)


# ---- skinny linear layers -------------------------------------------------------------
SKINNY_BATCHES = (1, 2, 3, 4, 8)
SKINNY_FWD_SHAPES = ((4, 8), (12, 520), (8, 8200), (256, 14336))
SKINNY_BWD_N = (4, 128, 132, 256, 260, 1000)  # around the data gradient's 128-row blocks
SKINNY_BWD_K = (8, 520, 4096)


@functools.lru_cache(maxsize=8)
def skinny_fwd_case(n: int, k: int):
    """x int64 [8, K] dense +-1 (batch b uses rows [:b]); W int64 [N, K] with one
    +-1 per column in a pseudo-random row, every row used; bias int64 [N] in
    {-3..3}.  y = x W^T (+ bias): each k is one term of one output per batch row."""
    g = gen(n * 7 + k)
    x = signs((8, k), g)
    rows = torch.randint(0, n, (k,), generator=g)
    rows[torch.randperm(k, generator=g)[:n]] = torch.arange(n)  # every row has an entry
    w = torch.zeros((n, k), dtype=I64)
    w[rows, torch.arange(k)] = signs((k,), g)
    bias = torch.randint(-3, 4, (n,), generator=g)
    return x, w, bias


def skinny_fwd_ref(x, w, bias, act: str) -> torch.Tensor:
    y = (x.double() @ w.double().t()).round().to(I64)
    if bias is not None:
        y = y + bias
    return y.clamp(min=0) if act == "relu" else y.clamp(0, 6) if act == "relu6" else y


@functools.lru_cache(maxsize=32)
def skinny_bwd_case(n: int, k: int):
    """dy, x in {-2..2} \\ {0} ([8, N], [8, K]; batch b uses rows [:b]); W [N, K]
    +-1 at about min(N, 32) rows per column, every row non-empty; yout [8, N]
    integers in {-3..9}, the source of the activation mask (see skinny_yout)."""
    g = gen(n * 11 + k)
    dy = nonzero_ints((8, n), g)
    x = nonzero_ints((8, k), g)
    keep = torch.rand((n, k), generator=g) < min(1.0, 32.0 / n)
    keep[torch.arange(n), torch.randint(0, k, (n,), generator=g)] = True
    w = signs((n, k), g) * keep
    yout = torch.randint(-3, 10, (8, n), generator=g)
    return dy, x, w, yout


def skinny_yout(yout: torch.Tensor, b: int) -> torch.Tensor:
    """yout for batch b: with more than one batch row, row n % b of column n is
    set to 3 (unmasked under relu and relu6), so every n keeps a non-zero g."""
    y = yout[:b].clone()
    if b > 1:
        cols = torch.arange(y.shape[1])
        y[cols % b, cols] = 3
    return y


def skinny_g(dy: torch.Tensor, yout: torch.Tensor | None, act: str) -> torch.Tensor:
    if yout is None or act == "none":
        return dy
    m = (yout > 0) if act == "relu" else ((yout > 0) & (yout < 6))
    return dy * m


def skinny_bwd_ref(g, x, w):
    """(dx [B,K], dW [N,K], db [N]) int64."""
    dx = (g.double() @ w.double()).round().to(I64)
    dw = (g.double().t() @ x.double()).round().to(I64)
    return dx, dw, g.sum(0)


# ---- depthwise 3x3 --------------------------------------------------------------------
def dw_out_hw(h: int, w: int, stride: int) -> tuple[int, int]:
    return (h - 1) // stride + 1, (w - 1) // stride + 1


def _dw_taps(x, stride, dil, oh, ow):
    """The nine shifted, strided views of x [N,C,H,W] (zero padding = dil)."""
    xp = torch.nn.functional.pad(x, (dil, dil, dil, dil))
    for k in range(9):
        kh, kw = divmod(k, 3)
        yield k, xp[:, :, kh * dil: kh * dil + (oh - 1) * stride + 1: stride,
                    kw * dil: kw * dil + (ow - 1) * stride + 1: stride]


def dw_fwd_ref(x, wt, stride, dil):
    """x int64 [N,C,H,W], wt int64 [C,9] -> y int64 [N,C,OH,OW]."""
    oh, ow = dw_out_hw(x.shape[2], x.shape[3], stride)
    y = torch.zeros((x.shape[0], x.shape[1], oh, ow), dtype=I64)
    for k, xs in _dw_taps(x, stride, dil, oh, ow):
        y += xs * wt[:, k].view(1, -1, 1, 1)
    return y


def dw_dgrad_ref(dy, wt, hw, stride, dil):
    h, w = hw
    n, c, oh, ow = dy.shape
    dxp = torch.zeros((n, c, h + 2 * dil, w + 2 * dil), dtype=I64)
    for k in range(9):
        kh, kw = divmod(k, 3)
        dxp[:, :, kh * dil: kh * dil + (oh - 1) * stride + 1: stride,
            kw * dil: kw * dil + (ow - 1) * stride + 1: stride] += dy * wt[:, k].view(1, -1, 1, 1)
    return dxp[:, :, dil: dil + h, dil: dil + w].contiguous()


def dw_wgrad_ref(dy, x, stride, dil):
    """-> int64 [9, C]."""
    oh, ow = dy.shape[2:]
    out = torch.zeros((9, x.shape[1]), dtype=I64)
    for k, xs in _dw_taps(x, stride, dil, oh, ow):
        out[k] = (xs * dy).sum((0, 2, 3))
    return out


def dw_dense_case(n, c, h, w, stride, dil, seed: int = 0):
    """x, wt [C,9], dy: int64 in {-2..2} (|sum of 9 products| <= 36)."""
    g = gen(seed + c * 3 + h)
    oh, ow = dw_out_hw(h, w, stride)
    x = torch.randint(-2, 3, (n, c, h, w), generator=g)
    wt = torch.randint(-2, 3, (c, 9), generator=g)
    dy = torch.randint(-2, 3, (n, c, oh, ow), generator=g)
    return x, wt, dy


def dw_wgrad_dense_case(n, c, h, w, stride, dil, seed: int = 0):
    """x, dy int64 in {-2..2} \\ {0}: every pixel is a non-zero term of the centre tap."""
    g = gen(seed + c * 5 + w)
    oh, ow = dw_out_hw(h, w, stride)
    return nonzero_ints((n, c, h, w), g), nonzero_ints((n, c, oh, ow), g)


def dw_wgrad_onehot_case(n, c, h, w, stride, dil, seed: int = 0):
    """One-hot x and dy for the bf16 weight gradient: dy at output pixel p is
    +-1 in channel fd(p); x is +-1 in a pseudo-random channel, except at p's
    centre-tap input pixel where it sits in fd(p) too, with the sign that makes
    the centre-tap terms of a channel alternate +1, -1, ... (their sum is 0 or
    1 whatever the pixel count, yet every pixel is a non-zero term)."""
    g = gen(seed + c * 7 + h)
    oh, ow = dw_out_hw(h, w, stride)
    fd = torch.randint(0, c, (n, oh, ow), generator=g)
    sd = signs((n, oh, ow), g)
    fx = torch.randint(0, c, (n, h, w), generator=g)
    sx = signs((n, h, w), g)
    flat = fd.reshape(-1)
    order = torch.argsort(flat, stable=True)
    start = torch.zeros(c + 1, dtype=I64)
    start[1:] = torch.bincount(flat, minlength=c).cumsum(0)
    rank = torch.empty_like(flat)
    rank[order] = torch.arange(flat.numel()) - start[flat[order]]
    alt = (1 - 2 * (rank % 2)).view(n, oh, ow)
    fx[:, ::stride, ::stride] = fd
    sx[:, ::stride, ::stride] = sd * alt
    x = _onehot(fx, sx, c).permute(0, 3, 1, 2).to(I64)
    dy = _onehot(fd, sd, c).permute(0, 3, 1, 2).to(I64)
    return x, dy


# (n, c, h, w, stride, dil), pixels P, what wgrad2_plan does with it
DW_WGRAD_CASES = [
    ((1, 8, 3, 4, 1, 1), 12, "one slab, ppt 1"),
    ((1, 16, 29, 33, 2, 1), 255, "one slab, ppt 1"),
    ((1, 8, 16, 16, 1, 1), 256, "one slab, ppt 1"),
    ((1, 24, 15, 20, 1, 2), 300, "one slab, ppt 2"),
    ((2, 8, 35, 10, 1, 1), 700, "one slab, ppt 3"),
    ((1, 8, 49, 81, 2, 2), 1025, "two slabs, the second holding one pixel"),
    ((1, 8, 150, 150, 1, 1), 22500, "22 slabs"),
    ((1, 8, 257, 257, 1, 1), 66049, "65 slabs: the reduce's unrolled loop and its tail"),
    ((1, 960, 132, 132, 1, 1), 17424, "ppt doubled to 8, 9 slabs"),
]
DW_FWD_SHAPES = ((2, 24, 7, 5), (1, 96, 33, 30))


def dw_plan(n, c, h, w, stride, dil) -> tuple[int, int]:
    """(pixels per thread, slabs) as dwconv.hip's wgrad2_plan chooses them."""
    oh, ow = dw_out_hw(h, w, stride)
    P = n * oh * ow
    if P <= 768:
        return (P + 255) // 256, 1
    ppt = 4
    sl = (P + 1023) // 1024
    while sl * (c // 8) > 2048 and ppt < 64:
        ppt *= 2
        sl = (P + 256 * ppt - 1) // (256 * ppt)
    return ppt, sl


# ---- forward split-K ------------------------------------------------------------------
SPLITK_KINDS = {  # the two shapes of test_conv_splitk_and_bf16_bias: n, c, h, cout, ks, pad, residual
    "3x3": (2, 512, 14, 512, 3, 1, False),
    "1x1_res": (3, 1024, 7, 256, 1, 0, True),
}


@functools.lru_cache(maxsize=2)
def splitk_case(kind: str):
    """x dense +-1 [N,H,W,C]; W [Cout,KS,KS,C] with one +-1 per reduction index
    (c, kh, kw) in a pseudo-random output channel; integer bias in {-3..3} and
    residual in {-4..4}; ref int64 [N,Cout,OH,OW] before the activation."""
    n, c, h, cout, ks, pad, has_res = SPLITK_KINDS[kind]
    g = gen(len(kind))
    x = signs((n, h, h, c), g)
    K = ks * ks * c
    co = torch.randint(0, cout, (K,), generator=g)
    w = torch.zeros((cout, K), dtype=I64)
    w[co, torch.arange(K)] = signs((K,), g)
    w = w.view(cout, ks, ks, c)
    bias = torch.randint(-3, 4, (cout,), generator=g)
    res = torch.randint(-4, 5, (n, h, h, cout), generator=g) if has_res else None
    y = torch.nn.functional.conv2d(x.permute(0, 3, 1, 2).double(), w.permute(0, 3, 1, 2).double(), padding=pad)
    y = y.round().to(I64) + bias.view(1, -1, 1, 1)
    if res is not None:
        y = y + res.permute(0, 3, 1, 2)
    return x, w, bias, res, y
