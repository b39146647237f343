"""Exact-integer tests of the forward convolution kernels that conv_plan.h plans
(native/kernels/conv_gemm.hip): every case of tests/_conv_exact.py runs through
vgpu_conv2d_nhwc_ws or vgpu_conv2d_post_nhwc_ws under its forced knobs and must
store the int64 reference bit for bit.

The C entry points are called directly (vgpu.ops.conv.conv2d caches the workspace
size by shape alone and would carry it across knob settings).  The output lies
between guard rows of 0xFF bytes and starts as 0xFF bytes itself (a bf16 NaN: a
row nobody stored differs from every reference); a split-K workspace starts as
NaNs between guard rows too.  tests/test_conv_exact_cpu.py shows, without a GPU,
that each case's reference satisfies the two conditions under which one lost term
changes a stored value, and that conv_plan names the kernel the case is there for."""
import gc

import pytest
import torch

import _conv_exact as X
from test_gpu_exact import _ptr, _stream

pytestmark = pytest.mark.gpu

BF, F32 = torch.bfloat16, torch.float32
GUARD_ROWS = 256  # the tallest tile: a row stored one tile off still lands in a guard


@pytest.fixture(scope="module")
def lib(gpu_build):
    from vgpu.native import load_kernels
    return load_kernels()


@pytest.fixture(scope="module", autouse=True)
def _release_memory():
    """Later tests in this process measure free HBM: hand back the cached cases and torch's blocks."""
    yield
    X.operands.cache_clear()
    X.reference.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


class Guarded:
    """rows x width elements between two runs of GUARD_ROWS rows, all 0xFF bytes at first."""

    def __init__(self, rows, width, dtype):
        size = torch.empty((), dtype=dtype).element_size()
        g = GUARD_ROWS * width * size
        self.raw = torch.full((2 * g + rows * width * size,), 0xFF, dtype=torch.uint8, device="cuda")
        self.head, self.tail = self.raw[:g], self.raw[g + rows * width * size:]
        self.t = self.raw[g:g + rows * width * size].view(dtype).view(rows, width)

    def intact(self):
        return bool((self.head == 0xFF).all()) and bool((self.tail == 0xFF).all())


def _dev(t, dtype):
    return None if t is None else t.to(dtype).cuda().contiguous()


def _report(case, got, want):
    """Where the stored bits part from the reference: (n, oh, ow, co) with M tile, N tile and row in the tile."""
    bad = (got.view(torch.int16) != want.view(torch.int16)).nonzero()
    oh, ow = case.out_hw
    lines = []
    for m, co in bad[:6].tolist() + bad[-2:].tolist():
        n, r = divmod(m, oh * ow)
        lines.append(f"(n {n}, oh {r // ow}, ow {r % ow}, co {co}) M tile {m // case.bm} row {m % case.bm} "
                     f"N tile {co // case.bn}: got {got[m, co].item()} want {want[m, co].item()}")
    rows, cols = bad[:, 0].unique(), bad[:, 1].unique()
    return (f"{case.name} ({case.what}; {case.kernel}): {bad.shape[0]} of {got.numel()} values differ, in "
            f"{rows.numel()} rows (M tiles {sorted(set((rows // case.bm).tolist()))[:12]}) and {cols.numel()} "
            f"channels (N tiles {sorted(set((cols // case.bn).tolist()))}); first six and last two:\n  "
            + "\n  ".join(lines))


@pytest.mark.parametrize("case", X.CASES, ids=[c.name for c in X.CASES])
def test_conv_exact(lib, case):
    n, h, w, c, cout, ks, stride, pad = case.shape
    o, r = X.operands(case), X.reference(case)
    x, wt, res = _dev(o["x"], BF), _dev(o["w"], BF), _dev(o["res"], BF)
    bias = _dev(o["bias"], BF if case.bias == "bf16" else F32)
    s, t, qs, qt = (_dev(o[k], F32) for k in ("s", "t", "qs", "qt"))
    want = r["want"].view(case.M, cout).cuda()
    y = Guarded(case.M, cout, BF)
    ws = None
    try:
        lib.vgpu_conv_set_tile_m(case.tile_m)
        lib.vgpu_conv_set_big(case.big)
        lib.vgpu_conv_set_halo(case.halo)
        lib.vgpu_conv_set_splitk(case.splitk)
        need = lib.vgpu_conv2d_workspace(n, h, w, c, cout, ks, stride, pad, int(case.pro))
        assert need == case.workspace
        if need:
            ws = Guarded(need // (cout * 4), cout, F32)
            assert bool(ws.t.isnan().all())
        before = lib.vgpu_conv_halo_launches()
        if case.post:
            rc = lib.vgpu_conv2d_post_nhwc_ws(_ptr(x), _ptr(wt), _ptr(y.t), _ptr(res), _ptr(qs), _ptr(qt), n, h, w, c,
                                              cout, stride, _ptr(ws.t) if ws else None, need, _stream())
        else:
            rc = lib.vgpu_conv2d_nhwc_ws(_ptr(x), _ptr(wt), _ptr(y.t), _ptr(res), _ptr(bias), _ptr(s), _ptr(t), n, h,
                                         w, c, cout, ks, stride, pad, case.act | (256 if case.bias == "bf16" else 0),
                                         _ptr(ws.t) if ws else None, need, _stream())
        halo_ran = lib.vgpu_conv_halo_launches() - before
    finally:
        lib.vgpu_conv_set_tile_m(0)
        lib.vgpu_conv_set_big(-1)
        lib.vgpu_conv_set_halo(-1)
        lib.vgpu_conv_set_splitk(-1)
    torch.cuda.synchronize()
    assert rc == 0
    assert halo_ran == (1 if case.family == "halo" else 0)
    assert y.intact(), "a store outside the output"
    if ws is not None:
        assert ws.intact(), "a store outside the workspace"
        assert not bool(ws.t.isnan().any()), f"{int(ws.t.isnan().sum())} partial sums unwritten"
    if not torch.equal(y.t.view(torch.int16), want.view(torch.int16)):
        raise AssertionError(_report(case, y.t, want))


def test_narrow_conv_with_a_residual_is_refused(lib):
    """No narrow kernel adds a residual: -1 before any launch, and y stays as it was."""
    case = next(c for c in X.CASES if c.name == "glds-narrow-bm64")
    n, h, w, c, cout, ks, stride, pad = case.shape
    o = X.operands(case)
    x, wt = _dev(o["x"], BF), _dev(o["w"], BF)
    res = torch.ones((case.M, cout), dtype=BF, device="cuda")
    y = Guarded(case.M, cout, BF)
    rc = lib.vgpu_conv2d_nhwc_ws(_ptr(x), _ptr(wt), _ptr(y.t), _ptr(res), None, None, None, n, h, w, c, cout, ks,
                                 stride, pad, 0, None, 0, _stream())
    torch.cuda.synchronize()
    assert rc == -1
    assert y.intact() and bool((y.t.view(torch.int16) == -1).all())
