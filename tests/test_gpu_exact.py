"""Bit-exact tests of the kernels whose reduction is long or split across
workgroups: small-integer operands make every product and every fp32 partial
sum exact in any order, so the result must EQUAL the int64 reference rounded
once to the output type -- one lost pixel, chunk, split or slab shows.  The
inputs and references are tests/_exact.py's; tests/test_exact_cpu.py proves on
the CPU that each reference is representable and sees every reduction index.
Direct library calls write into buffers with guard rows of 0xFF bytes (a NaN
for fp32 workspaces: a split nobody wrote poisons the sum)."""
import ctypes

import pytest
import torch

import _exact as E

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32 = torch.float32


class Guarded:
    """rows x width elements for a kernel to write, then 16 sentinel rows of 0xFF bytes
    (tests/test_gpu_decode.py's)."""

    def __init__(self, rows, width, dtype=BF, fill=None):
        n = rows * width * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((n // rows * (rows + 16),), 0xFF, dtype=torch.uint8, device="cuda")
        self.t = self.raw[:n].view(dtype).view(rows, width)
        self.tail = self.raw[n:]
        if fill is not None:
            self.t.copy_(fill)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    @property
    def nbytes(self):
        return self.t.numel() * self.t.element_size()

    def intact(self):
        return bool((self.tail == 0xFF).all())


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _same(got, ref, what):
    """torch.equal, saying where the two part."""
    ref = ref.to(got.device)
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape, got.dtype, ref.dtype)
    if torch.equal(got, ref):
        return
    bad = got.float() != ref.float()  # a NaN differs from everything
    at = bad.nonzero()
    first, last = at[0].tolist(), at[-1].tolist()
    raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} elements differ; first at {first}: got "
                         f"{got[tuple(first)].item()} want {ref[tuple(first)].item()}; last at {last}: got "
                         f"{got[tuple(last)].item()} want {ref[tuple(last)].item()}")


@pytest.fixture(scope="module")
def C(gpu_build):
    from vgpu.ops import conv
    return conv


@pytest.fixture(scope="module")
def lib(gpu_build):
    from vgpu.ops.linear import _lib
    return _lib()  # load_kernels() with the skinny entry points' argtypes bound


def _id(shape):
    return "x".join(map(str, shape))


# ---- 1. convolution weight gradient ---------------------------------------------------
def _splits(lib, shape):
    n, h, w, c, cout, ks, s, p = shape
    need = lib.vgpu_conv_wgrad_workspace(n, h, w, c, cout, ks, s, p)
    assert need >= 0
    return max(need // (cout * ks * ks * c * 4), 1), need


WGRAD_PARAMS = [pytest.param(sh, sp, mode, id=f"{_id(sh)}-{mode}")
                for sh, sp, _ in E.WGRAD_CASES for mode in E.wgrad_modes(sh)]


@pytest.mark.parametrize("shape,listed,mode", WGRAD_PARAMS)
def test_conv_wgrad_exact(C, lib, shape, listed, mode):
    """conv2d_wgrad on one-hot operands (every output pixel one +-1 product)
    and on the dense companion, for every tile, reduce variant, empty-split
    layout and both tap-fused kernels (E.WGRAD_CASES)."""
    n, h, w, c, cout, ks, s, p = shape
    splits, _ = _splits(lib, shape)
    # a case is listed for what this split count makes it exercise: if the
    # heuristic moves, pick a neighbouring size that restores it
    assert splits == listed, E.wgrad_plan(shape, splits)
    case = E.wgrad_case(shape, mode)
    dw = C.conv2d_wgrad(case.dy.cuda(), case.x.cuda(), ks, stride=s, padding=p)
    _same(dw, case.ref_as_weight(), f"dw [co, c, kh, kw], {E.wgrad_plan(shape, splits)}")


@pytest.mark.parametrize("shape", E.WGRAD_GUARDED, ids=_id)
def test_conv_wgrad_guarded_nan_workspace(lib, shape):
    """vgpu_conv_wgrad_nhwc called directly: dw and the split workspace have
    guard rows, and the workspace starts as NaNs -- a split whose (possibly
    empty) workgroup wrote no partial tile turns its sums into NaN."""
    n, h, w, c, cout, ks, s, p = shape
    splits, need = _splits(lib, shape)
    case = E.wgrad_case(shape, E.wgrad_modes(shape)[0])
    x, dy = case.x.cuda(), case.dy.cuda()
    ktot = ks * ks * c
    dw = Guarded(cout, ktot)
    ws = Guarded(splits, cout * ktot, F32)
    assert bool(ws.t.isnan().all()) and ws.nbytes >= need
    rc = lib.vgpu_conv_wgrad_nhwc(_ptr(dy), _ptr(x), dw.ptr, ws.ptr, need, n, h, w, c, cout, ks, s, p, _stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert dw.intact() and ws.intact()
    _same(dw.t, E.round_to(case.ref, BF).reshape(cout, ktot), f"dw [co, (kh, kw, c)], {E.wgrad_plan(shape, splits)}")
    if splits > 1:
        assert not bool(ws.t.isnan().any()), "a split left its partial tile unwritten"


def test_conv_wgrad_cases_cover_every_variant(lib):
    """With the split counts the library really gives, the cases above reach
    every tile shape, every wgrad_reduce_kernel<L>, empty trailing splits on
    every tile and both tap-fused kernels."""
    E.assert_wgrad_coverage([E.wgrad_plan(sh, _splits(lib, sh)[0]) for sh, _, _ in E.WGRAD_CASES])


def _db_ref(ref, bf16):
    return E.round_to(ref, BF if bf16 else F32).view(1, -1)


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("stride", [1, 2])
def test_bias_grad_reduce_exact(lib, stride, bf16):
    """vgpu_bias_grad_reduce alone: integer partials [slabs][c] at every slab
    count around the 16-lane and 64-slab strides of db_reduce_block."""
    for slabs in E.DB_SLABS:
        for c in E.DB_CHANNELS:
            part, ref = E.db_case(slabs, c, stride, bf16)
            db = Guarded(1, c, BF if bf16 else F32)
            rc = lib.vgpu_bias_grad_reduce(_ptr(part.cuda()), slabs, c, db.ptr, int(bf16), stride, _stream())
            assert rc == 0
            torch.cuda.synchronize()
            assert db.intact(), (slabs, c)
            _same(db.t, _db_ref(ref, bf16), f"db, {slabs} slabs x {c} channels")


@pytest.mark.parametrize("bf16", [False, True], ids=["fp32", "bf16"])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", [(1, 19, 21, 64, 64, 3, 1, 1), (1, 3, 5, 64, 64, 3, 1, 1)], ids=_id)
def test_bias_grad_rides_on_wgrad_exact(lib, shape, stride, bf16):
    """vgpu_conv_wgrad_db_nhwc: the bias gradient as extra blocks of the split
    weight gradient's reduce launch (4 splits), and as a launch of its own
    after a direct-write weight gradient; dw is held exact too."""
    n, h, w, c, cout, ks, s, p = shape
    splits, need = _splits(lib, shape)
    case = E.wgrad_case(shape, E.wgrad_modes(shape)[-1])
    x, dy = case.x.cuda(), case.dy.cuda()
    ktot = ks * ks * c
    want_dw = E.round_to(case.ref, BF).reshape(cout, ktot).cuda()
    for slabs in E.DB_SLABS:
        for dbc in E.DB_CHANNELS:
            part, ref = E.db_case(slabs, dbc, stride, bf16)
            db = Guarded(1, dbc, BF if bf16 else F32)
            dw = Guarded(cout, ktot)
            ws = Guarded(splits, cout * ktot, F32)
            rc = lib.vgpu_conv_wgrad_db_nhwc(_ptr(dy), _ptr(x), dw.ptr, ws.ptr, need, n, h, w, c, cout, ks, s, p,
                                             _ptr(part.cuda()), slabs, dbc, db.ptr, int(bf16), stride, _stream())
            assert rc == 0
            torch.cuda.synchronize()
            assert db.intact() and dw.intact() and ws.intact(), (slabs, dbc)
            _same(db.t, _db_ref(ref, bf16), f"db, {slabs} slabs x {dbc} channels")
            _same(dw.t, want_dw, f"dw with a {slabs} x {dbc} bias job")


# ---- 2. skinny linear layers ----------------------------------------------------------
_ACT = {"none": 0, "relu": 1, "relu6": 2}


def _bf(t):
    return t.to(BF).cuda().contiguous()


@pytest.mark.parametrize("nk", E.SKINNY_FWD_SHAPES, ids=_id)
@pytest.mark.parametrize("b", E.SKINNY_BATCHES)
def test_skinny_forward_exact(lib, b, nk):
    """vgpu_skinny_fwd at every batch instantiation: dense +-1 x against a
    weight with one +-1 per column, with and without an integer bias, every
    activation (integer sums make relu6's clamp exact)."""
    n, k = nk
    x8, w, bias = E.skinny_fwd_case(n, k)
    x, wd, bd = _bf(x8[:b]), _bf(w), _bf(bias)
    assert lib.vgpu_skinny_supported(b, n, k)
    for has_bias in (False, True):
        for act in _ACT:
            y = Guarded(b, n)
            rc = lib.vgpu_skinny_fwd(_ptr(x), _ptr(wd), _ptr(bd) if has_bias else None, y.ptr, b, n, k, _ACT[act],
                                     _stream())
            assert rc == 0
            torch.cuda.synchronize()
            assert y.intact()
            ref = E.skinny_fwd_ref(x8[:b], w, bias if has_bias else None, act)
            _same(y.t, E.round_to(ref, BF), f"y [b, n], bias {has_bias}, act {act}")


@pytest.mark.parametrize("n", E.SKINNY_BWD_N)
@pytest.mark.parametrize("b", E.SKINNY_BATCHES)
def test_skinny_backward_exact(lib, b, n):
    """vgpu_skinny_dgrad and vgpu_skinny_backward: dx over a ragged block of
    rows, exactly one and two blocks, just over each, and eight, dW and db,
    without an activation and with the mask taken from an integer yout; K on
    both sides of the dx split-sum's grid (E.SKINNY_BWD_K)."""
    for k in E.SKINNY_BWD_K:
        dy8, x8, w, yout8 = E.skinny_bwd_case(n, k)
        dy, x, yout = dy8[:b], x8[:b], E.skinny_yout(yout8, b)
        dyd, xd, wd, youtd = _bf(dy), _bf(x), _bf(w), _bf(yout)
        need = lib.vgpu_skinny_dgrad_workspace(b, n, k)
        assert need == (n + 127) // 128 * b * k * 4
        for act in _ACT:
            yo = None if act == "none" else youtd
            dx, dw, db = (E.round_to(t, BF) for t in E.skinny_bwd_ref(E.skinny_g(dy, yout, act), x, w))
            what = f"K {k}, act {act}"
            # the data gradient alone
            gdx, ws = Guarded(b, k), Guarded(need // (b * k * 4), b * k, F32)
            rc = lib.vgpu_skinny_dgrad(_ptr(dyd), _ptr(yo), _ptr(wd), gdx.ptr, ws.ptr, need, b, n, k, _ACT[act],
                                       _stream())
            assert rc == 0
            torch.cuda.synchronize()
            assert gdx.intact() and ws.intact(), what
            _same(gdx.t, dx, f"dgrad dx [b, k], {what}")
            # the whole backward: dx's split sum rides in the weight gradient's grid
            gdx, gdw, gdb = Guarded(b, k), Guarded(n, k), Guarded(1, n)
            ws = Guarded(need // (b * k * 4), b * k, F32)
            rc = lib.vgpu_skinny_backward(_ptr(dyd), _ptr(yo), _ptr(xd), _ptr(wd), gdx.ptr, gdw.ptr, gdb.ptr, ws.ptr,
                                          need, b, n, k, _ACT[act], _stream())
            assert rc == 0
            torch.cuda.synchronize()
            assert gdx.intact() and gdw.intact() and gdb.intact() and ws.intact(), what
            _same(gdx.t, dx, f"backward dx [b, k], {what}")
            _same(gdw.t, dw, f"backward dW [n, k], {what}")
            _same(gdb.t, db.view(1, -1), f"backward db [n], {what}")


# ---- 3. depthwise 3x3 -----------------------------------------------------------------
def _cl(t):
    return t.to(BF).cuda().contiguous(memory_format=E.CL)


@pytest.mark.parametrize("dil", [1, 2])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("shape", E.DW_FWD_SHAPES, ids=_id)
def test_dwconv_forward_dgrad_exact(gpu_build, shape, stride, dil):
    """Depthwise forward and data gradient on integers in {-2..2} (|sum| <= 36),
    from the fp32 [9, C] filter and from the module's bf16 [C, 1, 3, 3]."""
    from vgpu.ops import dwconv as D
    n, c, h, w = shape
    x, wt, dy = E.dw_dense_case(n, c, h, w, stride, dil)
    y = E.round_to(E.dw_fwd_ref(x, wt, stride, dil), BF)
    dx = E.round_to(E.dw_dgrad_ref(dy, wt, (h, w), stride, dil), BF)
    xd, dyd = _cl(x), _cl(dy)
    filters = {"fp32 [9, C]": wt.t().contiguous().float().cuda(), "bf16 [C, 1, 3, 3]": wt.view(c, 1, 3, 3).to(BF).cuda()}
    for name, f in filters.items():
        _same(D.dwconv3(xd, f, stride, dil), y, f"y, filter {name}")
        _same(D.dwconv3_dgrad(dyd, f, (h, w), stride, dil), dx, f"dx, filter {name}")


@pytest.mark.parametrize("case", E.DW_WGRAD_CASES, ids=lambda c: _id(c[0]))
def test_dwconv_wgrad_exact(gpu_build, case):
    """Depthwise weight gradient at every plan of wgrad2_plan (one slab with 1,
    2 or 3 pixels a thread; 2, 22, 65 slabs; pixels per thread doubled): fp32
    [9, C] from dense integers, the bf16 module layout from one-hot operands."""
    from vgpu.ops import dwconv as D
    (n, c, h, w, stride, dil), pixels, what = case
    need = D._lib().vgpu_dwconv3_wgrad_workspace(n, h, w, c, stride, dil)
    ppt, slabs = E.dw_plan(n, c, h, w, stride, dil)
    assert need == (0 if slabs == 1 else slabs * 9 * c * 4), (need, ppt, slabs)  # the plan the case is listed for
    x, dy = E.dw_wgrad_dense_case(n, c, h, w, stride, dil)
    ref = E.dw_wgrad_ref(dy, x, stride, dil)
    _same(D.dwconv3_wgrad(_cl(dy), _cl(x), stride, dil), E.round_to(ref, F32), f"dw fp32 [9, C], {what}")
    if pixels > E.DENSE_PIXELS:
        x, dy = E.dw_wgrad_onehot_case(n, c, h, w, stride, dil)
        ref = E.dw_wgrad_ref(dy, x, stride, dil)
    got = D.dwconv3_wgrad(_cl(dy), _cl(x), stride, dil, "module")
    _same(got, E.round_to(ref.t().reshape(c, 1, 3, 3), BF), f"dw bf16 [C, 1, 3, 3], {what}")


# ---- 4. forward split-K ---------------------------------------------------------------
@pytest.mark.parametrize("act", ["none", "relu"])
@pytest.mark.parametrize("splits", [-1, 3, 7])
@pytest.mark.parametrize("kind", list(E.SPLITK_KINDS))
def test_conv_splitk_exact(C, kind, splits, act):
    """The two shapes of test_conv_splitk_and_bf16_bias under the heuristic and
    3 / 7 forced splits: dense +-1 input, a weight with one +-1 per reduction
    index, integer bias (fp32 and bf16) and residual."""
    n, c, h, cout, ks, pad, has_res = E.SPLITK_KINDS[kind]
    x, w, bias, res, y = E.splitk_case(kind)
    ref = E.round_to(y.clamp(min=0) if act == "relu" else y, BF)
    xd, wd = E.to_nchw_cl(x).cuda(), E.to_nchw_cl(w).cuda()
    resd = E.to_nchw_cl(res).cuda() if has_res else None
    C.set_splitk(splits)
    try:
        need = C.load_kernels().vgpu_conv2d_workspace(n, h, h, c, cout, ks, 1, pad, 0)
        got = [C.conv2d(xd, wd, bias.to(dt).cuda(), padding=pad, act=act, residual=resd) for dt in (F32, BF)]
    finally:
        C.set_splitk(-1)
    assert need > 0, "the shape did not split"
    for g, dt in zip(got, ("fp32", "bf16")):
        _same(g, ref, f"y [n, co, oh, ow], {dt} bias")
