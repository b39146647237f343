"""Exact-integer inputs, int64 references and the case table for the forward
convolution kernels that native/kernels/conv_plan.h plans (conv_gemm.hip through
vgpu_conv2d_nhwc_ws and vgpu_conv2d_post_nhwc_ws).  Pure CPU torch.

    y   = act(conv(pro(x), w) + bias + residual),   pro(x) = relu(x * s[c] + t[c])
    out = relu(bf16(y) * qs[co] + qt[co])           (the post entry point; else out = y)

Activations, weights and the residual are small-integer bf16, s / t / qs / qt
integer-valued fp32, the bias integer-valued fp32 or bf16.  Every product, every
partial sum, the prologue value and the post value are then integers that fp32 and
bf16 hold exactly, so a kernel must reproduce the reference bit for bit in any
summation order.  Two conditions make the comparison see a single lost term;
tests/test_conv_exact_cpu.py asserts both on the REFERENCE of every case:

1. representability: max|value| <= 128 for the conv sum, y and out (all integers
   up to 256 are exact in bf16: a wrong integer differs or rounds to >= 256);
2. visibility: for every output pixel, every 64-wide K step (tap x 64-channel
   block; four taps x 16 channels in the narrow form) and every 64-wide block of
   output channels, one or more terms pro(x)[m, k] * w[co, k] are non-zero.  Taps
   in the padding are excused.  A lost (M tile, K step, N tile) triple therefore
   changes some stored value.

Operand schemes:
  sparse_w     x dense +-1; w one +-1 per reduction index in each 64-channel output
               block, the 64 indices of a K step going to 64 different channels, so
               each output is a sum of exactly one term per K step.
  sparse_both  for the deepest K (C > 2048 with 3x3): x also has one non-zero channel
               per pixel per 64-channel block.  With a prologue the other channels
               read relu(t): t is 1 on two channels of each block and <= 0 elsewhere.
  dense        the shallow companion of every family: x and w dense in {-2..2},
               K <= 576, compared with the reference rounded once to bf16 (condition 1
               is then |sum| < 2**24: the fp32 sums stay exact, only the store rounds).

Prologue parameters: |s| in {1, 2} and t in {-1..2} with t > -|s|, so no channel is
zero at all pixels, channels with t <= 0 clamp where x * s is negative, and channels
with t > 0 turn a zero-padding tap (or an M-tail row) into a non-zero term should the
prologue be applied to it.  Post parameters: qs in {-1, 1, 2}, qt in {-3..3}.
"""
from __future__ import annotations

import dataclasses
import functools

import torch

from _exact import BF16_EXACT, FP32_EXACT, I64, gen, out_hw, round_to, signs

F64 = torch.float64
ACTS = ("none", "relu", "relu6")
BIASES = ("none", "f32", "bf16")


def _b(v) -> str:
    return "true" if v else "false"


# The kernel names as a launch trace prints them (scripts/conv_plan_trace.py).
def k_gemm(ks, bm, bn, res):
    return f"conv_gemm_kernel<{ks}, {bm}, {bn}, {_b(res)}>"


def k_pro(ks, bm, bn, res):
    return f"conv_pro_kernel<{ks}, {bm}, {bn}, {_b(res)}>"


def k_glds(ks, bm, bn, res, csm=0, split=False, post=False):
    return f"conv_glds_kernel<{ks}, {bm}, {bn}, {_b(res)}, {csm}, 0, {_b(split)}, {_b(post)}>"


def k_big(res):
    return f"conv_big_kernel<{_b(res)}, 4>"


def k_halo(bm):
    return f"conv_halo_kernel<{bm}, 128, {bm * 3 // 2}, 0>"


def k_reduce(post):
    return f"splitk_reduce_kernel<{_b(post)}>"


def all_planned_kernels() -> set[str]:
    """The 62 ST = 0 entries of conv_kernel()'s tables and both split-K reduces."""
    tiles = [(ks, bm, bn) for ks in (1, 3) for bm in (64, 128) for bn in (64, 128)]
    names = {k(ks, bm, bn, r) for k in (k_gemm, k_pro, k_glds) for ks, bm, bn in tiles for r in (False, True)}
    names |= {k_glds(ks, 64, bn, False, split=True) for ks in (1, 3) for bn in (64, 128)}
    names |= {k_glds(1, bm, bn, True, post=True) for bm in (64, 128) for bn in (64, 128)}
    names |= {k_glds(4, bm, 64, False, csm=16) for bm in (64, 128)}
    names |= {k_big(False), k_big(True), k_halo(128), k_halo(256)}
    assert len(names) == 62
    return names | {k_reduce(False), k_reduce(True)}


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    family: str          # gemm pro glds split post big halo (split: glds with a split count)
    shape: tuple         # N H W C Cout KS stride pad
    kernel: str          # the kernel conv_plan must name, at any CU count
    bm: int              # its tile (for the mismatch report)
    bn: int
    what: str
    pro: bool = False
    res: bool = False
    bias: str = "none"
    act: int = 0         # 0 none, 1 relu, 2 relu6
    post: bool = False
    scheme: str = "sparse_w"
    tile_m: int = 0      # the four knobs, forced so that the plan does not depend on the CU count
    big: int = 0
    halo: int = 0
    splitk: int = 0
    splits: int = 1      # the split count the plan ends up with (ragged counts round down)

    @property
    def knobs(self) -> dict:
        return dict(tile_m=self.tile_m, big=self.big, halo=self.halo, splitk=self.splitk)

    @property
    def out_hw(self) -> tuple[int, int]:
        n, h, w, c, cout, ks, s, p = self.shape
        return out_hw(h, w, ks, s, p)

    @property
    def M(self) -> int:
        oh, ow = self.out_hw
        return self.shape[0] * oh * ow

    @property
    def ktiles(self) -> int:
        return self.shape[5] ** 2 * self.shape[3] // 64

    @property
    def workspace(self) -> int:
        """Bytes vgpu_conv2d_workspace must answer under the case's knobs."""
        return self.splits * self.M * self.shape[4] * 4 if self.splits > 1 else 0

    @property
    def reduce(self) -> str | None:
        return k_reduce(self.post) if self.splits > 1 else None

    @property
    def plan_family(self) -> str:
        return {"split": "glds", "post": "glds"}.get(self.family, self.family)


# ---- operands -------------------------------------------------------------------------
def _seed(case: Case) -> int:
    return sum((i + 1) * v for i, v in enumerate(case.shape)) * 8 + case.act + 3 * BIASES.index(case.bias)


def _sparse_weights(cout: int, ks: int, c: int, g) -> torch.Tensor:
    """int64 [Cout, KS, KS, C]: per 64-channel output block and reduction index k one
    +-1, in channel (k + r[block, k // 64]) % 64 of the block."""
    K = ks * ks * c
    k = torch.arange(K)
    w = torch.zeros((cout, K), dtype=I64)
    for j in range(cout // 64):
        r = torch.randint(0, 64, ((K + 63) // 64,), generator=g)
        w[64 * j + (k + r[k // 64]) % 64, k] = signs((K,), g)
    return w.view(cout, ks, ks, c)


def _prologue(c: int, g, sparse: bool):
    """(s, t) int64 [C]; see the module docstring."""
    s = signs((c,), g) * torch.randint(1, 3, (c,), generator=g)
    if sparse:
        t = -torch.randint(0, 2, (c,), generator=g) * (s.abs() == 2)
        for b in range(c // 64):
            t[64 * b + torch.randperm(64, generator=g)[:2]] = 1
    else:
        t = torch.randint(-1, 3, (c,), generator=g)
        t = torch.where(t <= -s.abs(), torch.zeros_like(t), t)   # t > -|s|
        t = torch.where((s.abs() == 2) & (t == 2), torch.ones_like(t), t)  # pro(x) <= 3
    return s, t


def _onehot_blocks(shape, c: int, s, g) -> torch.Tensor:
    """x int64 [*shape, C] with one non-zero channel per 64-channel block, of the sign
    that the prologue scale s (or None) keeps positive."""
    nb = c // 64
    pixel = torch.arange(int(torch.tensor(shape).prod())).view(*shape, 1)
    # (pixel + r[block]) % 64: from 64 pixels up every channel is the non-zero one somewhere
    hot = (pixel + torch.randint(0, 64, (nb,), generator=g)) % 64 + 64 * torch.arange(nb)
    val = signs((*shape, nb), g) if s is None else torch.sign(s)[hot]
    return torch.zeros((*shape, c), dtype=I64).scatter_(-1, hot, val)


@functools.lru_cache(maxsize=2)
def operands(case: Case) -> dict:
    """int64 tensors: x [N,H,W,C], w [Cout,KS,KS,C], and where the case has them
    bias [Cout], res [N,OH,OW,Cout], s / t [C], qs / qt [Cout]."""
    n, h, wd, c, cout, ks, stride, pad = case.shape
    oh, ow = case.out_hw
    g = gen(_seed(case))
    o = dict.fromkeys(("bias", "res", "s", "t", "qs", "qt"))
    if case.pro:
        o["s"], o["t"] = _prologue(c, g, case.scheme == "sparse_both")
    if case.scheme == "dense":
        o["x"] = torch.randint(-2, 3, (n, h, wd, c), generator=g)
        o["w"] = torch.randint(-2, 3, (cout, ks, ks, c), generator=g)
    else:
        o["x"] = _onehot_blocks((n, h, wd), c, o["s"], g) if case.scheme == "sparse_both" else signs((n, h, wd, c), g)
        o["w"] = _sparse_weights(cout, ks, c, g)
    if case.bias != "none":
        o["bias"] = torch.randint(-8, 9, (cout,), generator=g)
    if case.res:
        o["res"] = torch.randint(-4, 5, (n, oh, ow, cout), generator=g)
    if case.post:
        o["qs"] = torch.tensor([-1, 1, 2])[torch.randint(0, 3, (cout,), generator=g)]
        o["qt"] = torch.randint(-3, 4, (cout,), generator=g)
    return o


def prologue_value(case: Case, o: dict) -> torch.Tensor:
    """pro(x), int64 [N,H,W,C] (x itself without a prologue)."""
    return (o["x"] * o["s"] + o["t"]).clamp(min=0) if case.pro else o["x"]


# ---- reference ------------------------------------------------------------------------
@functools.lru_cache(maxsize=2)
def reference(case: Case) -> dict:
    """int64 [N,OH,OW,Cout]: conv (the bare sum), pre (+ bias + residual), y (after the
    activation), out (the post value, or y), and want: bf16, what the kernel must store."""
    n, h, wd, c, cout, ks, stride, pad = case.shape
    o = operands(case)
    px = prologue_value(case, o)
    conv = torch.nn.functional.conv2d(px.permute(0, 3, 1, 2).to(F64), o["w"].permute(0, 3, 1, 2).to(F64),
                                      stride=stride, padding=pad)
    conv = conv.round().to(I64).permute(0, 2, 3, 1).contiguous()
    pre = conv.clone()
    if o["bias"] is not None:
        pre += o["bias"]
    if o["res"] is not None:
        pre += o["res"]
    y = pre if case.act == 0 else pre.clamp(min=0) if case.act == 1 else pre.clamp(0, 6)
    r = dict(conv=conv, pre=pre, y=y, out=y)
    if case.post:
        # the post epilogue reads y as it was rounded to bf16 (exact but for the dense companion)
        yb = round_to(y, torch.bfloat16).to(F64)
        r["out"] = (yb * o["qs"] + o["qt"]).clamp(min=0)
        r["post_pre"] = yb * o["qs"] + o["qt"]
    r["want"] = round_to(r["out"], torch.bfloat16)
    return r


def representable(case: Case, r: dict) -> bool:
    """Condition 1."""
    bound = FP32_EXACT - 1 if case.scheme == "dense" else BF16_EXACT
    return all(int(r[k].abs().max()) <= bound for k in ("conv", "pre", "y", "out"))


def visible(case: Case, o: dict) -> bool:
    """Condition 2."""
    n, h, wd, c, cout, ks, stride, pad = case.shape
    oh, ow = case.out_hw
    cg = min(c, 64)                                  # channels of one tap in a K step
    pnz = torch.nn.functional.pad((prologue_value(case, o) != 0).float(), (0, 0, pad, pad, pad, pad))
    inside = torch.nn.functional.pad(torch.ones((h, wd)), (pad, pad, pad, pad))
    # per 64-channel output block: is there a weight at (tap, c)?
    wnz = (o["w"] != 0).view(cout // 64, 64, ks, ks, c).any(1).float()
    seen, real = [], []                              # per tap: [N,OH,OW,C/cg,Cout/64] and [OH,OW]
    for kh in range(ks):
        for kw in range(ks):
            rows = slice(kh, kh + (oh - 1) * stride + 1, stride)
            cols = slice(kw, kw + (ow - 1) * stride + 1, stride)
            xs = pnz[:, rows, cols].reshape(n, oh, ow, c // cg, cg)
            seen.append(torch.einsum("nhwbc,jbc->nhwbj", xs, wnz[:, kh, kw].reshape(-1, c // cg, cg)) > 0)
            real.append(inside[rows, cols] > 0)
    seen, real = torch.stack(seen), torch.stack(real)
    per = 64 // cg                                   # taps per K step: 1, or 4 in the narrow form
    seen = seen.view(-1, per, *seen.shape[1:]).any(1)
    real = real.view(-1, per, oh, ow).any(1)
    return bool((seen | ~real.view(-1, 1, oh, ow, 1, 1)).all())


# ---- the case table -------------------------------------------------------------------
def _epilogues(i: int) -> dict:
    """One bias / activation combination for the i-th case of a sweep; relu6 always with
    a bias, so that short reductions too have values above 6."""
    act = (i // 3 + i) % 3
    return dict(bias=BIASES[i % 3 or (act == 2)], act=act)


def _cross(res_options=(False, True)):
    return [dict(bias=b, act=a, res=r) for r in res_options for b in BIASES for a in range(3)]


def _tag(e: dict) -> str:
    return f"{e['bias']}-{ACTS[e['act']]}" + ("-res" if e.get("res") else "")


def _gemm_cases() -> list[Case]:
    out = []
    shapes = {  # (KS, BN) -> shape, scheme, what
        (1, 64): ((2, 7, 9, 64, 64, 1, 1, 0), "sparse_w", "one K step, Cout 64"),
        (1, 128): ((1, 13, 10, 128, 128, 1, 1, 0), "sparse_w", "two K steps"),
        (3, 64): ((2, 7, 9, 128, 64, 3, 1, 1), "sparse_w", "3x3, Cout 64"),
        (3, 128): ((1, 9, 8, 2112, 128, 3, 1, 1), "sparse_both", "3x3 with C 2112 > 2048"),
    }
    i = 0
    for (ks, bn), (shape, scheme, what) in shapes.items():
        for bm in (64, 128):
            for res in (False, True):
                out.append(Case(f"gemm-{ks}x{ks}-bm{bm}-bn{bn}-res{int(res)}", "gemm", shape,
                                k_gemm(ks, bm, bn, res), bm, bn, what, pro=True, res=res, scheme=scheme,
                                tile_m=bm, **_epilogues(i)))
                i += 1
    out += [
        Case("gemm-padded-1x1", "gemm", (1, 6, 7, 192, 192, 1, 1, 1), k_gemm(1, 64, 64, True), 64, 64,
             "a padded 1x1: three K steps, every border output reads only padding", pro=True, res=True,
             bias="f32", act=1, tile_m=64),
        Case("gemm-cout64-k5", "gemm", (1, 13, 10, 320, 64, 1, 1, 0), k_gemm(1, 128, 64, False), 128, 64,
             "Cout 64 with five K steps", pro=True, bias="bf16", act=2, tile_m=128),
        # persistent: 5 workgroups of 32 KiB (64x64) / 3 of 48 KiB (128x64) fit a CU's 160 KiB, so at most
        # 256 * 5 = 1280 / 256 * 3 = 768 are resident: 4113 and 2321 tiles are more than three each, and odd
        # where the grid is a multiple of 8
        Case("gemm-persistent-bm64", "gemm", (1, 513, 513, 64, 64, 1, 1, 0), k_gemm(1, 64, 64, True), 64, 64,
             "persistent, 4113 tiles of one K step, last tile one row", pro=True, res=True, bias="f32", act=1,
             tile_m=64),
        Case("gemm-persistent-bm128", "gemm", (1, 545, 545, 64, 64, 1, 1, 0), k_gemm(1, 128, 64, True), 128, 64,
             "persistent, 2321 tiles of one K step, last tile 65 rows", pro=True, res=True, act=2, bias="bf16",
             tile_m=128),
        Case("gemm-dense", "gemm", (1, 5, 6, 64, 64, 3, 1, 1), k_gemm(3, 64, 64, True), 64, 64, "dense companion",
             pro=True, res=True, bias="f32", act=1, scheme="dense", tile_m=64),
    ]
    for e in _cross():
        out.append(Case("gemm-cross-" + _tag(e), "gemm", (2, 7, 9, 128, 64, 3, 1, 1), k_gemm(3, 64, 64, e["res"]), 64,
                        64, "epilogue cross", pro=True, tile_m=64, **e))
    return out


def _pro_cases() -> list[Case]:
    table = [  # KS BM BN RES shape what
        (1, 64, 64, False, (2, 7, 9, 192, 192, 1, 1, 0), "three K steps, the minimum"),
        (1, 64, 64, True, (1, 5, 5, 256, 320, 1, 1, 0), "four K steps, M < one tile, Cout 320"),
        (1, 64, 128, False, (1, 9, 11, 320, 128, 1, 2, 0), "five K steps (odd remainder), strided 1x1"),
        (1, 64, 128, True, (2, 9, 9, 192, 256, 1, 1, 0), "three tiles, two N tiles"),
        (1, 128, 64, False, (1, 13, 10, 320, 192, 1, 1, 0), "five K steps, parameters from LDS"),
        (1, 128, 64, True, (1, 13, 10, 2048, 192, 1, 1, 0), "C 2048 fills the LDS parameter copy"),
        (1, 128, 128, False, (1, 9, 9, 2048, 128, 1, 1, 0), "C 2048, M < one tile"),
        (1, 128, 128, True, (2, 15, 13, 256, 128, 1, 2, 0), "strided 1x1 on odd H and W"),
        (3, 64, 64, False, (3, 3, 3, 64, 192, 3, 1, 1), "3x3 images: 8 of 9 taps are padding in the corners"),
        (3, 64, 64, True, (2, 7, 9, 128, 192, 3, 1, 1), "18 K steps"),
        (3, 64, 128, False, (2, 9, 11, 64, 128, 3, 2, 1), "strided 3x3"),
        (3, 64, 128, True, (1, 13, 10, 64, 256, 3, 1, 1), "three M tiles, two N tiles"),
        (3, 128, 64, False, (15, 3, 3, 64, 320, 3, 1, 1), "3x3 images across two tiles"),
        (3, 128, 64, True, (2, 7, 9, 64, 192, 3, 1, 1), "M < one tile"),
        (3, 128, 128, False, (1, 13, 10, 128, 128, 3, 1, 1), "18 K steps, two tiles"),
        (3, 128, 128, True, (2, 3, 3, 64, 128, 3, 1, 1), "3x3 images, M = 18"),
    ]
    out = [Case(f"pro-{ks}x{ks}-bm{bm}-bn{bn}-res{int(res)}", "pro", shape, k_pro(ks, bm, bn, res), bm, bn, what,
                pro=True, res=res, tile_m=bm, **_epilogues(i))
           for i, (ks, bm, bn, res, shape, what) in enumerate(table)]
    out.append(Case("pro-dense", "pro", (1, 5, 6, 64, 128, 3, 1, 1), k_pro(3, 64, 128, False), 64, 128,
                    "dense companion", pro=True, bias="bf16", act=2, scheme="dense", tile_m=64))
    for e in _cross():
        out.append(Case("pro-cross-" + _tag(e), "pro", (2, 7, 9, 192, 192, 1, 1, 0), k_pro(1, 64, 64, e["res"]), 64,
                        64, "epilogue cross", pro=True, tile_m=64, **e))
    return out


def _glds_cases() -> list[Case]:
    table = [  # KS BM BN RES shape what
        (1, 64, 64, False, (1, 35, 11, 64, 64, 1, 1, 0), "7 tiles, M % 64 = 1"),
        (1, 64, 64, True, (1, 7, 73, 64, 64, 1, 1, 0), "8 tiles, M % 64 = 63, one K step: early residual"),
        (1, 64, 128, False, (1, 17, 19, 128, 256, 1, 2, 0), "stride 2 on odd H and W"),
        (1, 64, 128, True, (1, 27, 19, 256, 128, 1, 1, 0), "9 tiles, four K steps: late residual"),
        (1, 128, 64, False, (1, 1, 127, 64, 64, 1, 1, 0), "one tile, M % 128 = 127"),
        (1, 128, 64, True, (1, 1, 257, 128, 192, 1, 1, 0), "9 tiles (3 x 3), M % 128 = 1, late residual"),
        (1, 128, 128, False, (1, 27, 109, 64, 128, 1, 1, 0), "23 tiles, M % 128 = 127"),
        (1, 128, 128, True, (1, 13, 10, 64, 128, 1, 1, 0), "one K step: early residual"),
        (3, 64, 64, False, (1, 7, 9, 64, 64, 3, 1, 1), "one tile, M % 64 = 63"),
        (3, 64, 64, True, (1, 15, 17, 64, 192, 3, 2, 1), "stride 2 on odd H and W"),
        (3, 64, 128, False, (1, 21, 21, 64, 128, 3, 1, 1), "7 tiles; the halo kernel is switched off"),
        (3, 64, 128, True, (1, 5, 13, 128, 128, 3, 1, 1), "M % 64 = 1"),
        (3, 128, 64, False, (1, 27, 109, 64, 64, 3, 1, 1), "23 tiles, M % 128 = 127"),
        (3, 128, 64, True, (1, 7, 9, 64, 64, 3, 1, 1), "M < one tile"),
        (3, 128, 128, False, (1, 9, 57, 64, 256, 3, 1, 1), "10 tiles, M % 128 = 1"),
        (3, 128, 128, True, (2, 8, 8, 64, 128, 3, 1, 1), "exactly one tile"),
    ]
    out = [Case(f"glds-{ks}x{ks}-bm{bm}-bn{bn}-res{int(res)}", "glds", shape, k_glds(ks, bm, bn, res), bm, bn, what,
                res=res, tile_m=bm, **_epilogues(i))
           for i, (ks, bm, bn, res, shape, what) in enumerate(table)]
    out += [
        Case("glds-narrow-bm64", "glds", (1, 10, 12, 16, 64, 4, 1, 0), k_glds(4, 64, 64, False, csm=16), 64, 64,
             "narrow stem form, M = 63", tile_m=64),
        Case("glds-narrow-bm128", "glds", (1, 10, 12, 16, 64, 4, 1, 0), k_glds(4, 128, 64, False, csm=16), 128, 64,
             "narrow stem form, M < one tile", bias="f32", act=1, tile_m=128),
        Case("glds-narrow-padded", "glds", (2, 10, 9, 16, 64, 4, 1, 1), k_glds(4, 64, 64, False, csm=16), 64, 64,
             "narrow stem form with padding, three tiles", bias="bf16", act=2, tile_m=64),
        Case("glds-narrow-bm128-tiles", "glds", (2, 13, 14, 16, 64, 4, 1, 0), k_glds(4, 128, 64, False, csm=16), 128,
             64, "narrow stem form, two tiles of 128", tile_m=128),
        Case("glds-dense", "glds", (1, 5, 6, 64, 64, 3, 1, 1), k_glds(3, 64, 64, True), 64, 64, "dense companion",
             res=True, bias="f32", act=1, scheme="dense", tile_m=64),
    ]
    for e in _cross():
        out.append(Case("glds-cross-" + _tag(e), "glds", (1, 5, 13, 128, 128, 3, 1, 1),
                        k_glds(3, 64, 128, e["res"]), 64, 128, "epilogue cross", tile_m=64, **e))
    return out


def _split_cases() -> list[Case]:
    def case(name, shape, ks, bn, splitk, splits, what, **kw):
        return Case(name, "split", shape, k_glds(ks, 64, bn, False, split=True), 64, bn, what, splitk=splitk,
                    splits=splits, **kw)
    out = [
        case("split-3x3-bn128", (2, 7, 7, 512, 128, 3, 1, 1), 3, 128, 7, 7, "72 K steps in 7 splits: 11, ..., 6",
             bias="f32", act=1),
        case("split-3x3-bn64", (1, 7, 9, 128, 192, 3, 1, 1), 3, 64, 4, 4, "18 K steps in 4 splits: 5, 5, 5, 3",
             bias="bf16", act=2, res=True),
        case("split-1x1-bn64", (1, 9, 9, 1344, 64, 1, 1, 0), 1, 64, 5, 5, "21 K steps in 5 splits: a last split of one",
             res=True),
        case("split-1x1-bn128", (3, 7, 7, 1024, 256, 1, 1, 0), 1, 128, 3, 3, "16 K steps in 3 splits: 6, 6, 4",
             bias="f32", act=2),
        case("split-post-bn64", (1, 9, 9, 512, 64, 1, 1, 0), 1, 64, 2, 2, "the post epilogue in the reduce", res=True,
             post=True),
        case("split-post-bn128", (2, 7, 7, 576, 128, 1, 1, 0), 1, 128, 2, 2,
             "the post epilogue in the reduce, 9 K steps: 5, 4", res=True, post=True),
        case("split-dense", (1, 7, 9, 64, 64, 3, 1, 1), 3, 64, 2, 2, "dense companion", bias="f32", act=1, res=True,
             scheme="dense"),
    ]
    for e in _cross():
        out.append(case("split-cross-" + _tag(e), (1, 7, 9, 512, 128, 1, 1, 0), 1, 128, 2, 2,
                        "epilogue cross in the reduce", **e))
    return out


def _post_cases() -> list[Case]:
    table = [  # BM BN shape what
        (64, 64, (1, 5, 13, 64, 64, 1, 1, 0), "M % 64 = 1, one K step"),
        (64, 128, (1, 9, 9, 128, 128, 1, 1, 0), "two K steps, ragged M"),
        (128, 64, (1, 13, 10, 192, 192, 1, 1, 0), "three N tiles, M % 128 = 2"),
        (128, 128, (1, 15, 13, 256, 128, 1, 2, 0), "strided, M < one tile"),
    ]
    out = [Case(f"post-bm{bm}-bn{bn}", "post", shape, k_glds(1, bm, bn, True, post=True), bm, bn, what, res=True,
                post=True, tile_m=bm) for bm, bn, shape, what in table]
    out.append(Case("post-dense", "post", (1, 5, 13, 576, 64, 1, 1, 0), k_glds(1, 64, 64, True, post=True), 64, 64,
                    "dense companion", res=True, post=True, scheme="dense", tile_m=64))
    return out


def _big_cases() -> list[Case]:
    out = [
        Case("big-k128-m1", "big", (1, 1, 1, 128, 256, 1, 1, 0), k_big(False), 256, 256,
             "K 128: four steps of 32, the ring's minimum; M = 1", big=1, bias="f32"),
        Case("big-k192-m255", "big", (1, 15, 17, 192, 512, 1, 1, 0), k_big(True), 256, 256,
             "K 192, M = 255, two N tiles, bias + relu6 + residual", big=1, res=True, bias="f32", act=2),
        Case("big-k1024-m257", "big", (1, 1, 257, 1024, 768, 1, 1, 0), k_big(False), 256, 256,
             "K 1024, M = 257, three N tiles", big=1, bias="bf16", act=1),
        Case("big-k128-m257-res", "big", (1, 257, 1, 128, 256, 1, 1, 0), k_big(True), 256, 256,
             "K 128 with a residual, M = 257", big=1, res=True),
        Case("big-dense", "big", (1, 3, 5, 512, 256, 1, 1, 0), k_big(True), 256, 256, "dense companion", big=1,
             res=True, bias="f32", act=1, scheme="dense"),
    ]
    for e in _cross():
        out.append(Case("big-cross-" + _tag(e), "big", (1, 15, 17, 1024, 256, 1, 1, 0), k_big(e["res"]), 256, 256,
                        "epilogue cross", big=1, **e))
    return out


def _halo_cases() -> list[Case]:
    def case(name, shape, mode, what, **kw):
        bm = 256 if mode == 2 else 128
        return Case(name, "halo", shape, k_halo(bm), bm, 128, what, halo=mode, **kw)
    out = [
        case("halo-128-w19", (1, 7, 19, 64, 128, 3, 1, 1), 3, "W 19: 190 of 191 halo pixels", bias="f32", act=1),
        case("halo-256-w38", (1, 7, 38, 64, 128, 3, 1, 1), 2, "W 38: 380 of 383 halo pixels", bias="bf16", act=2),
        case("halo-128-w1", (2, 70, 1, 64, 128, 3, 1, 1), 3, "W 1; tile 0 spans two images"),
        case("halo-256-w1", (4, 70, 1, 128, 128, 3, 1, 1), 2, "W 1; tile 0 spans four images", act=1),
        case("halo-128-h1", (9, 1, 17, 64, 256, 3, 1, 1), 3, "H 1; two N tiles", bias="f32"),
        case("halo-256-h1", (9, 1, 38, 64, 128, 3, 1, 1), 2, "H 1; BM 256"),
        case("halo-128-3images", (3, 3, 17, 64, 128, 3, 1, 1), 3, "tile 0 spans three images"),
        case("halo-128-2images", (2, 5, 19, 64, 128, 3, 1, 1), 3, "tile 0 spans two images", act=2, bias="f32"),
        case("halo-256-2images", (2, 5, 38, 64, 128, 3, 1, 1), 2, "tile 0 spans two images, BM 256"),
        case("halo-128-nmajor", (1, 5, 5, 512, 512, 3, 1, 1), 3, "N-major: a 4.5 MiB filter; M < one tile",
             bias="bf16", act=1),
        case("halo-1x1-images", (5, 1, 1, 64, 128, 3, 1, 1), 3, "H = W = 1: every tap but the centre is padding"),
        case("halo-dense", (1, 6, 16, 64, 128, 3, 1, 1), 3, "dense companion", bias="f32", act=1, scheme="dense"),
    ]
    for e in _cross(res_options=(False,)):
        out.append(case("halo-cross-" + _tag(e), (1, 7, 19, 64, 128, 3, 1, 1), 3, "epilogue cross", **e))
    return out


CASES: list[Case] = (_gemm_cases() + _pro_cases() + _glds_cases() + _split_cases() + _post_cases() + _big_cases()
                     + _halo_cases())
assert len({c.name for c in CASES}) == len(CASES)
# small enough for vgpu.ops.conv.conv2d_ref (fp32) in the CPU test
SMALL = [c for c in CASES if c.M * c.shape[4] * c.ktiles <= 1 << 22]


def images_spanned(case: Case) -> set[int]:
    """How many images the rows of each M tile come from."""
    oh, ow = case.out_hw
    return {(min(m0 + case.bm, case.M) - 1) // (oh * ow) - m0 // (oh * ow) + 1 for m0 in range(0, case.M, case.bm)}


def assert_coverage(rows: list[tuple[Case, dict]]) -> None:
    """The per-family edges, from the fields of each case's plan (conv_plan.h through
    native/tests/conv_plan_capi.cpp): rows = [(case, plan)]."""
    def of(fam):
        return [(c, p) for c, p in rows if c.family == fam and c.scheme != "dense"]

    def last_split(c, p):
        return c.ktiles - (p["splits"] - 1) * p["kper"]

    g = of("gemm")
    assert {c.ktiles for c, _ in g} >= {1, 2}
    assert any(c.shape[4] == 64 and c.ktiles > 2 for c, _ in g)
    assert any(c.shape[5] == 1 and c.shape[7] > 0 for c, _ in g) and any(c.shape[3] > 2048 for c, _ in g)
    for bm, resident in ((64, 256 * 5), (128, 256 * 3)):
        pers = [(c, p) for c, p in g if p["BM"] == bm and p["nM"] * p["nN"] > 3 * resident]
        assert pers, f"no persistent case on BM {bm}"
        assert all((p["nM"] * p["nN"]) % 8 and c.ktiles <= 2 and c.M % bm and c.res for c, p in pers)
    pr = of("pro")
    assert {c.ktiles for c, _ in pr} >= {3, 4, 5}
    assert any(c.shape[3] == 2048 and p["BM"] == 128 for c, p in pr)
    assert any(c.shape[1:3] == (3, 3) and c.shape[5] == 3 and c.shape[7] == 1 for c, _ in pr)
    assert any(c.M < p["BM"] for c, p in pr) and any(c.shape[5] == 1 and c.shape[6] == 2 for c, _ in pr)
    assert {c.shape[4] for c, p in pr if p["BN"] == 64} >= {192, 320}
    gl = [(c, p) for c, p in of("glds") if not p["CSM"]]
    assert any(c.res and c.ktiles == 1 for c, _ in gl) and any(c.res and c.ktiles >= 2 for c, _ in gl)
    assert {p["nM"] * p["nN"] for _, p in gl} >= {1, 7, 8, 9, 23}
    assert any(c.shape[6] == 2 and c.shape[1] % 2 and c.shape[2] % 2 for c, _ in gl)
    assert {c.M % p["BM"] for c, p in gl if p["BM"] == 64} >= {1, 63}
    assert {c.M % p["BM"] for c, p in gl if p["BM"] == 128} >= {1, 127}
    assert {p["BM"] for c, p in of("glds") if p["CSM"] == 16} == {64, 128}
    sp = of("split")
    assert all(p["splits"] > 1 and p["BM"] == 64 for _, p in sp)
    assert any((c.ktiles, p["splits"], p["kper"], last_split(c, p)) == (72, 7, 11, 6) for c, p in sp)
    assert any(last_split(c, p) == 1 and p["kper"] > 1 for c, p in sp)
    assert any(c.bias != "none" and c.res and c.act for c, _ in sp)
    assert {p["BN"] for c, p in sp if c.post and c.shape[3] >= 512} == {64, 128}
    po = of("post")
    assert {(p["BM"], p["BN"]) for _, p in po} == {(64, 64), (64, 128), (128, 64), (128, 128)}
    assert any(c.M % p["BM"] for c, p in po)
    bg = of("big")
    assert {c.shape[3] for c, _ in bg} >= {128, 192, 1024} and {c.M for c, _ in bg} >= {1, 255, 257}
    assert any(p["nN"] > 1 for _, p in bg) and any(c.bias != "none" and c.act == 2 and c.res for c, _ in bg)
    ha = of("halo")
    assert any(p["BM"] == 128 and c.shape[2] == 19 for c, p in ha)
    assert any(p["BM"] == 256 and c.shape[2] == 38 for c, p in ha)
    assert any(c.shape[2] == 1 for c, _ in ha) and any(c.shape[1] == 1 for c, _ in ha)
    assert set().union(*(images_spanned(c) for c, _ in ha)) >= {1, 2, 3}
    assert any(p["nmajor"] for _, p in ha) and any(c.M < p["BM"] for c, p in ha)
    # every family: a dense companion and the bias x activation (x residual) cross
    for fam in ("gemm", "pro", "glds", "split", "post", "big", "halo"):
        mine = [c for c, _ in rows if c.family == fam]
        assert any(c.scheme == "dense" and c.ktiles <= 9 for c in mine), fam
        if fam == "post":
            continue  # the post entry point takes no bias and no activation
        want = {(b, a, r) for b in BIASES for a in range(3) for r in ((False,) if fam == "halo" else (False, True))}
        shapes = {c.shape for c in mine}
        assert any(want <= {(c.bias, c.act, c.res) for c in mine if c.shape == s} for s in shapes), fam
