"""The inputs of tests/test_gpu_exact.py, checked without a GPU: every case's
integer reference is representable in the kernel's output type (condition 1)
and every index of its reduction is a non-zero term of some output (condition
2), and the scatter / shift references of tests/_exact.py equal dense fp64
PyTorch on the small cases.  Changing a shape there must keep these true."""
import pytest
import torch
import torch.nn.functional as F

import _exact as E

I64 = torch.int64


def _wgrad_params():
    return [pytest.param(sh, mode, id="x".join(map(str, sh)) + "-" + mode)
            for sh, _, _ in E.WGRAD_CASES for mode in E.wgrad_modes(sh)]


@pytest.mark.parametrize("shape,mode", _wgrad_params())
def test_wgrad_case_is_representable_and_visible(shape, mode):
    case = E.wgrad_case(shape, mode)
    n, h, w, c, cout, ks, s, p = shape
    oh, ow = E.out_hw(h, w, ks, s, p)
    peak = int(case.ref.abs().max())
    share = float((case.ref != 0).float().mean())
    print(f"{shape} {mode}: max|ref| {peak}, non-zero outputs {share:.2%}")
    assert 0 < peak <= E.BF16_EXACT
    assert int(case.x_nhwc.abs().max()) <= 2 and int(case.dy_nhwc.abs().max()) <= 2
    if mode == "onehot":
        assert E.wgrad_visible(case)
        assert bool(((case.x_nhwc != 0).sum(-1) == 1).all()) and bool(((case.dy_nhwc != 0).sum(-1) == 1).all())
    else:
        # the companion: dense operands on <= 32 pixels that span the pixel range
        live = (case.dy_nhwc.reshape(n * oh * ow, cout) != 0)
        rows = live.any(-1).nonzero().flatten()
        assert rows.numel() <= E.DENSE_PIXELS and int(rows[0]) == 0 and int(rows[-1]) == n * oh * ow - 1
        assert bool(live[rows].all()) and bool((case.x_nhwc != 0).all())
        if n * oh * ow <= E.DENSE_PIXELS:
            assert E.wgrad_visible(case)
        assert share > 0.9


SMALL_WGRAD = [(1, 9, 7, 64, 64, 3, 1, 1), (2, 9, 11, 64, 128, 3, 2, 1), (1, 7, 9, 128, 64, 1, 2, 0),
               (1, 3, 5, 64, 64, 3, 1, 1), (1, 3, 5, 64, 64, 1, 2, 0), (1, 15, 17, 64, 64, 3, 1, 1),
               (1, 19, 21, 64, 64, 3, 1, 1)]


@pytest.mark.parametrize("shape", SMALL_WGRAD, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", ["onehot", "dense"])
def test_wgrad_scatter_reference_equals_fp64(shape, mode):
    case = E.wgrad_onehot(shape) if mode == "onehot" else E.wgrad_dense(shape)
    ks, s, p = shape[5:]
    assert torch.equal(case.ref, E.wgrad_dense_ref(case.x_nhwc, case.dy_nhwc, ks, s, p))
    x, dy = case.x, case.dy  # what the kernel is given: the same integers, bf16 channels_last
    assert x.is_contiguous(memory_format=E.CL) and torch.equal(x.permute(0, 2, 3, 1).to(torch.int8), case.x_nhwc)
    assert torch.equal(dy.permute(0, 2, 3, 1).to(torch.int8), case.dy_nhwc)


def test_wgrad_cases_list_every_variant():
    """With the split counts listed (the GPU test holds them against the
    library's), the cases reach every tile, every reduce instantiation, an
    empty trailing split on every tile, and both tap-fused kernels."""
    E.assert_wgrad_coverage([E.wgrad_plan(sh, sp) for sh, sp, _ in E.WGRAD_CASES])
    for sh in E.WGRAD_GUARDED:
        assert any(sh == c[0] for c in E.WGRAD_CASES)


@pytest.mark.parametrize("bf16", [False, True])
@pytest.mark.parametrize("stride", [1, 2])
def test_db_partials(stride, bf16):
    for slabs in E.DB_SLABS:
        for c in E.DB_CHANNELS:
            part, ref = E.db_case(slabs, c, stride, bf16)
            assert part.shape == (slabs, c, stride)
            v = part[:, :, 0]
            assert torch.equal(v, v.round()) and bool((v != 0).any(1).all())  # integers; every slab visible
            assert torch.equal(ref, v.double().sum(0).to(I64))
            assert int(ref.abs().max()) <= (E.BF16_EXACT if bf16 else E.FP32_EXACT - 1)
            if stride == 2:
                assert bool((part[:, :, 1] != part[:, :, 1].round()).all())  # the skipped lanes would show


@pytest.mark.parametrize("n,k", E.SKINNY_FWD_SHAPES)
def test_skinny_forward_cases(n, k):
    x, w, bias = E.skinny_fwd_case(n, k)
    assert bool(((w != 0).sum(0) == 1).all()) and bool((w != 0).any(1).all())  # every k, every row
    assert bool((x.abs() == 1).all())
    for b in E.SKINNY_BATCHES:
        for bb in (None, bias):
            ref = E.skinny_fwd_ref(x[:b], w, bb, "none")
            print(f"fwd N={n} K={k} B={b} bias={bb is not None}: max|ref| {int(ref.abs().max())}")
            assert int(ref.abs().max()) <= E.BF16_EXACT
            assert torch.equal(ref, F.linear(x[:b].double(), w.double(), None if bb is None else bb.double()).to(I64))
            r6 = E.skinny_fwd_ref(x[:b], w, bb, "relu6")
            assert int(r6.min()) == 0 and int(r6.max()) <= 6
            assert torch.equal(E.skinny_fwd_ref(x[:b], w, bb, "relu"), ref.clamp(min=0))
    if n * 8 >= 64:  # enough outputs for both clamps of relu6 to act
        ref = E.skinny_fwd_ref(x, w, bias, "none")
        assert bool((ref > 6).any()) and bool((ref < 0).any())


@pytest.mark.parametrize("n", E.SKINNY_BWD_N)
@pytest.mark.parametrize("k", E.SKINNY_BWD_K)
def test_skinny_backward_cases(n, k):
    dy8, x8, w, yout8 = E.skinny_bwd_case(n, k)
    assert bool((w != 0).any(1).all())
    for b in E.SKINNY_BATCHES:
        dy, x = dy8[:b], x8[:b]
        yout = E.skinny_yout(yout8, b)
        for act in ("none", "relu", "relu6"):
            g = E.skinny_g(dy, None if act == "none" else yout, act)
            dx, dw, db = E.skinny_bwd_ref(g, x, w)
            peak = max(int(t.abs().max()) for t in (dx, dw, db))
            assert peak <= E.BF16_EXACT, (b, act, peak)
            if act == "none" or b > 1:
                assert bool((g != 0).any(0).all())      # every n is a non-zero term of dx
            if act != "none":
                masked = (g == 0)
                assert bool(masked.any()) or n * b < 16  # the mask does something
            # plain fp64 autograd of the same integers
            xr, wr = x.double().requires_grad_(), w.double().requires_grad_()
            (F.linear(xr, wr) * g.double()).sum().backward()
            assert torch.equal(dx, xr.grad.to(I64)) and torch.equal(dw, wr.grad.to(I64))


def test_skinny_backward_dx_job_grid_is_straddled():
    """The dx split-sum riding in the weight-gradient grid loops over B*K/8
    items with gridDim.x * 256 threads: the cases sit on both sides."""
    below = above = False
    for k in E.SKINNY_BWD_K:
        for b in E.SKINNY_BATCHES:
            threads = ((k // 8 + 255) // 256) * 256
            below |= b * k // 8 < threads
            above |= b * k // 8 > threads
    assert below and above


def _dw_torch(x, wt, dy, stride, dil):
    xr = x.double().requires_grad_()
    wr = wt.double().view(-1, 1, 3, 3).requires_grad_()
    y = F.conv2d(xr, wr, stride=stride, padding=dil, dilation=dil, groups=x.shape[1])
    y.backward(dy.double())
    return y.detach().to(I64), xr.grad.to(I64), wr.grad.view(-1, 9).t().to(I64)


@pytest.mark.parametrize("shape", E.DW_FWD_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dil", [1, 2])
def test_dw_dense_references_equal_fp64(shape, stride, dil):
    n, c, h, w = shape
    x, wt, dy = E.dw_dense_case(n, c, h, w, stride, dil)
    y, dx, dw = _dw_torch(x, wt, dy, stride, dil)
    assert torch.equal(E.dw_fwd_ref(x, wt, stride, dil), y)
    assert torch.equal(E.dw_dgrad_ref(dy, wt, (h, w), stride, dil), dx)
    assert torch.equal(E.dw_wgrad_ref(dy, x, stride, dil), dw)
    assert int(y.abs().max()) <= 36 and int(dx.abs().max()) <= 36 and 0 < int(y.abs().max())


@pytest.mark.parametrize("case", E.DW_WGRAD_CASES, ids=lambda c: "x".join(map(str, c[0])))
def test_dw_wgrad_cases(case):
    (n, c, h, w, stride, dil), pixels, what = case
    oh, ow = E.dw_out_hw(h, w, stride)
    assert n * oh * ow == pixels
    small = pixels * c <= 1 << 16
    # fp32 [9, C]: dense operands, every pixel a non-zero term of the centre tap
    x, dy = E.dw_wgrad_dense_case(n, c, h, w, stride, dil)
    ref = E.dw_wgrad_ref(dy, x, stride, dil)
    assert bool((x != 0).all()) and bool((dy != 0).all())
    assert int(ref.abs().max()) < E.FP32_EXACT and 4 * pixels < E.FP32_EXACT
    if small:
        assert torch.equal(ref, _dw_torch(x, torch.zeros(c, 9, dtype=I64), dy, stride, dil)[2])
    # bf16 [C, 1, 3, 3]: dense up to 32 pixels, one-hot beyond
    if pixels > E.DENSE_PIXELS:
        x, dy = E.dw_wgrad_onehot_case(n, c, h, w, stride, dil)
        assert bool(((dy != 0).sum(1) == 1).all()) and bool(((x != 0).sum(1) == 1).all())
        centre = x[:, :, ::stride, ::stride] * dy
        assert bool((centre != 0).any(1).all())  # every output pixel is a non-zero centre-tap term
        ref = E.dw_wgrad_ref(dy, x, stride, dil)
        if small:
            assert torch.equal(ref, _dw_torch(x, torch.zeros(c, 9, dtype=I64), dy, stride, dil)[2])
    print(f"{case[0]} P={pixels}: bf16 max|ref| {int(ref.abs().max())}")
    assert 0 < int(ref.abs().max()) <= E.BF16_EXACT


def test_dw_wgrad_cases_reach_every_plan():
    plans = {E.dw_plan(*c[0]) for c in E.DW_WGRAD_CASES}
    assert {(1, 1), (2, 1), (3, 1), (4, 2), (4, 22), (4, 65), (8, 9)} <= plans
    # the reduce's four-way unrolled loop runs while k + 48 < slabs: once for some lanes of 65, never below 49
    assert any(sl > 64 for _, sl in plans) and any(1 < sl <= 48 for _, sl in plans)


@pytest.mark.parametrize("kind", list(E.SPLITK_KINDS))
def test_splitk_case(kind):
    x, w, bias, res, y = E.splitk_case(kind)
    n, c, h, cout, ks, pad, has_res = E.SPLITK_KINDS[kind]
    assert bool(((w.reshape(cout, -1) != 0).sum(0) == 1).all())  # every (kh, kw, c) feeds one output channel
    assert bool((x.abs() == 1).all()) and (res is not None) == has_res
    assert int(y.abs().max()) <= E.BF16_EXACT
    assert bool((y < 0).any()) and bool((y > 0).any())  # relu has something to clamp
