"""The references of tests/_step_exact.py, without a GPU: each one equals
PyTorch's own operation in float64, each listed shape reaches the launch path
it is listed for, and the bit bounds that make the GPU comparison exact hold
(the case builders assert them; building every case here runs them all)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _exact as E
import _step_exact as S

F64 = torch.float64


# ---- cross-entropy ---------------------------------------------------------------------
def _xent_cases():
    seen = set()
    for family, kind, rows, c, bchw, ignore in S.xent_layout_cases():
        key = (family, rows, c, ignore, None)
        if key not in seen:
            seen.add(key)
            yield key
    yield ("selection", 65, 65, -100, 0)
    yield ("selection", 257, 21, 5, 0)
    for kind, rows, c, bchw in S.xent_op_cases():
        yield ("selection", rows, c, -100, 8)


@pytest.mark.parametrize("key", sorted(set(_xent_cases()), key=str), ids=lambda k: "-".join(map(str, k)))
def test_xent_reference_is_torch_float64(key):
    family, rows, c, ignore, keep = key
    case = S.xent_case(family, rows, c, ignore, keep)
    x = case.x.clone().requires_grad_()
    # PyTorch on the CPU raises for a target outside [0, C) that is not ignore_index;
    # the kernel ignores such a row, so PyTorch is handed ignore_index in its place
    t = torch.where(S.xent_valid(case.t, c, ignore), case.t, torch.tensor(ignore))
    per_row = F.cross_entropy(x, t, ignore_index=ignore, reduction="none").detach()
    assert torch.allclose(per_row, case.loss_rows, atol=1e-12, rtol=0)
    if case.valid == 0:
        assert np.isnan(case.out[0]) and case.out[1] == 0 and not bool(case.grad.any())
        return
    loss = F.cross_entropy(x, t, ignore_index=ignore)
    loss.backward()
    loss = loss.detach()
    assert abs(float(loss) - float(case.loss_rows.sum()) / case.valid) <= 1e-12
    assert torch.allclose(x.grad * case.valid, case.grad, atol=1e-12, rtol=0)
    # the fp32 mean and reciprocal are the float64 ones rounded once
    assert case.out[1] == np.float32(1.0 / case.valid)
    if case.exact_loss:
        assert case.out[0] == np.float32(float(case.loss_rows.sum())) / np.float32(case.valid)
        assert float(case.loss_rows.sum()) < S.FP32_EXACT
    else:
        assert abs(float(case.out[0]) - float(loss)) <= 1e-6


def test_xent_selection_sweeps():
    """Every hot class and every target kind the issue lists is present, and
    the last row of every case is valid with a non-zero loss."""
    case = S.xent_case("selection", 100, 1000, S.xent_inside_ignore(1000))
    hot = case.x.argmax(1)
    assert set(hot.tolist()) == {0, 63, 64, 255, 256, 999}
    t, ign = case.t, case.ignore
    assert bool((t == hot).any()) and bool(((t != hot) & S.xent_valid(t, 1000, ign)).any())
    for v in (ign, -100, -1, 1000, 255):
        assert bool((t == v).any()), v
    assert 0 <= ign < 1000
    d = S.xent_case("selection", 257, 21, 255)
    assert bool((d.t == 255).any()) and not bool(S.xent_valid(d.t, 21, 255)[d.t == 255].any())
    for family, kind, rows, c, bchw, ignore in S.xent_layout_cases():
        k = S.xent_case(family, rows, c, ignore)
        assert bool(S.xent_valid(k.t, c, ignore)[rows - 1])
        if family == "selection" and c > 2:
            assert float(k.loss_rows[rows - 1]) >= 256


def test_xent_shapes_reach_their_paths():
    for (rows, c), path in S.XENT_SHAPES.items():
        assert S.xent_path(rows, c) == path, (rows, c)
    assert {S.xent_path(r, c) for r, c in S.XENT_PADDED} == {"narrow", "small", "wide"}
    # both sides of both thresholds
    assert S.xent_path(256, 64) == "narrow" and S.xent_path(65, 65) == "wide" and S.xent_path(64, 65) == "small"
    paths = {}
    for kind, shapes in S.XENT_MAPS.items():
        for b, c, h, w in shapes:
            paths[(kind, b * h * w, c)] = S.xent_path(b * h * w, c)
    assert paths == {("cl", 70, 21): "narrow", ("cl", 18, 65): "small", ("nchw", 70, 21): "narrow",
                     ("nchw", 297, 64): "narrow"}
    assert 297 > S.XENT_THREADS
    # ragged narrow blocks, and an exact multiple
    narrow = [r for (r, c), p in S.XENT_SHAPES.items() if p == "narrow"]
    assert {r % 256 for r in narrow} >= {0, 1, 255}
    # the partials start at an even index and end with the workspace
    for rows in (1, 255, 256, 257, 513):
        assert S.xent_workspace(rows, 21) == ((rows + 1) // 2) * 2 + 2 * -(-rows // 256)
    assert S.xent_workspace(65, 65) == 65


def test_xent_ragged_block_double_count_would_show():
    """A CPU model of the narrow kernel's block partials gives the case's out;
    counting the spare lanes of a ragged last block (they re-read row
    rows - 1, which every case keeps valid) changes out[1], and out[0] with it."""
    ragged = 0
    for family, kind, rows, c, bchw, ignore in S.xent_layout_cases():
        if family != "selection" or S.xent_path(rows, c) != "narrow":
            continue
        case = S.xent_case(family, rows, c, ignore)
        ok = S.xent_valid(case.t, c, ignore)
        assert np.array_equal(S.xent_narrow_out(case.loss_rows, ok), case.out)
        wrong = S.xent_narrow_out(case.loss_rows, ok, count_spare=True)
        if rows % S.XENT_THREADS:
            ragged += 1
            assert wrong[1] != case.out[1], (rows, c)
            assert float(case.loss_rows.sum()) == 0 or wrong[0] != case.out[0], (rows, c)
        else:
            assert np.array_equal(wrong, case.out)
    assert ragged >= 6


@pytest.mark.parametrize("kind,bchw", [("dense", None), ("padded", None), ("cl", (2, 21, 5, 7)), ("nchw", (2, 21, 5, 7))])
def test_xent_layouts_address_like_torch(kind, bchw):
    """The storage offsets the kernel header's formula gives are the ones of a
    torch tensor of that memory format (rows = (b, h, w))."""
    rows, c = (70, 21)
    lay = S.xent_layout(kind, rows, c, bchw)
    vals = torch.arange(rows * c, dtype=F64).view(rows, c)
    t = S.xent_tensor(lay, S.xent_store(lay, vals, F64, -1.0))
    as_rows = t if t.dim() == 2 else t.permute(0, 2, 3, 1).reshape(rows, c)
    assert torch.equal(as_rows, vals)
    if kind == "cl":
        assert t.is_contiguous(memory_format=torch.channels_last)
    elif kind != "padded":
        assert t.is_contiguous()
    else:
        assert t.stride() == (c + S.PAD_COLS, 1)


# ---- SGD ------------------------------------------------------------------------------
@pytest.mark.parametrize("hp", list(S.SGD_HP))
@pytest.mark.parametrize("name", list(S.SGD_SIZES))
def test_sgd_reference(name, hp):
    """Three steps from a first step, and one continuing step from integer
    momentum: every intermediate is float32-exact (asserted inside), and step
    1 is torch.optim.SGD on float64 copies."""
    kw = S.SGD_HP[hp]
    for p0, m0, gs in S.sgd_case(name)[:8]:
        states = S.sgd_run_ref(p0, gs, kw)
        S.sgd_run_ref(p0, gs[:1], kw, m0)
        assert len(states) == S.SGD_STEPS
        q = p0.to(F64).clone().requires_grad_()
        opt = torch.optim.SGD([q], **kw)
        q.grad = gs[0].to(F64)
        opt.step()
        p1, m1 = S.sgd_step_ref(p0.to(F64), gs[0].to(F64), None, kw, True)
        assert torch.equal(q.detach(), p1) and torch.equal(opt.state[q]["momentum_buffer"], m1)
        assert S.bf16_exact(p1) and S.bf16_exact(m1)  # the first step rounds nothing
        # a continuing step too
        q.grad = gs[1].to(F64)
        opt.step()
        p2, m2 = S.sgd_step_ref(p1, gs[1].to(F64), m1, kw, False)
        assert torch.allclose(q.detach(), p2, atol=1e-12, rtol=0)
        assert torch.allclose(opt.state[q]["momentum_buffer"], m2, atol=1e-12, rtol=0)


def test_sgd_sizes_reach_the_tails():
    sizes = S.SGD_SIZES["sizes"]
    assert 2056 // 8 == 257 and sizes[-1] % S.SGD_CHUNK == 2056
    assert {n % S.SGD_CHUNK for n in sizes} >= {8, 2048, 2056, 8184, 0}
    assert S.sgd_blocks(sizes) == [0, 1, 2, 3, 4, 5, 7, 11]
    assert all(len(v) <= S.SGD_MAX_SEG for v in S.SGD_SIZES.values())
    assert len(S.SGD_SIZES["48x8"]) == len(S.SGD_SIZES["big_ends"]) == S.SGD_MAX_SEG
    assert S.sgd_blocks(S.SGD_SIZES["48x8"]) == list(range(49))
    b = S.sgd_blocks(S.SGD_SIZES["big_ends"])
    assert b[:3] == [0, 3, 4] and b[-3:] == [48, 49, 51]
    # a CPU model of the kernel's segment search covers every element once; searching with
    # `<` in place of `<=` leaves all of every segment but the first untouched, or its first chunk
    for name, sz in S.SGD_SIZES.items():
        assert S.sgd_covered(sz) == list(sz), name
        short = S.sgd_covered(sz, strict=True)
        assert short[0] == sz[0] and all(s < n for s, n in zip(short[1:], sz[1:])), name


def test_sgd_class_case_is_bf16_exact():
    """The optimizer-class case: 50 tensors the native path takes, one it does
    not; for its step counts every intermediate is exact in bf16 as well, so
    PyTorch's bf16 arithmetic on the 51st tensor is held to the same reference."""
    shapes = S.SGD_CLASS_SHAPES
    assert len(shapes) == 51 and sum(int(np.prod(s)) % 8 == 0 for s in shapes) == 50
    assert shapes[0] == (16, 8, 3, 3) and int(np.prod(shapes[-1])) % 8 != 0
    for hp, steps in S.SGD_CLASS_RUNS.items():
        for p0, gs in S.sgd_class_case(steps):
            S.sgd_run_ref(p0, gs, S.SGD_HP[hp], exact=S.bf16_exact)


# ---- training max pool -----------------------------------------------------------------
@pytest.mark.parametrize("kind", S.POOL_KINDS)
@pytest.mark.parametrize("ksp,shape", S.POOL_SMALL, ids=lambda v: "x".join(map(str, v)))
def test_pool_loop_reference(ksp, shape, kind):
    x, dy = S.pool_inputs(ksp, shape, kind)
    y, tap, dx = S.pool_loop_ref(x, dy, ksp)
    k, s, p = ksp
    assert float(dx.abs().max()) <= 4 * k * k and int(tap.max()) < k * k
    assert float(dx.sum()) == float(dy.sum())  # every dy lands on one pixel
    if kind == "nan":
        assert bool(y.isnan().any()) and bool((y == -float("inf")).any())
        nan_in = x.isnan().any()
        assert nan_in
        return
    ty, ttap, tdx = S.pool_torch_ref(x, dy, ksp)
    assert torch.equal(y, ty) and torch.equal(tap, ttap) and torch.equal(dx, tdx)
    if k > 1:  # the last maximum in place of the first (>= for >) moves taps and dx, not y
        y2, tap2, dx2 = S.pool_loop_ref(x, dy, ksp, strict=False)
        assert torch.equal(y2, y) and not torch.equal(tap2, tap) and not torch.equal(dx2, dx)
    if kind == "const" and ksp == (3, 1, 1):
        assert float((dx / dy.abs().max()).abs().max()) <= 4 and int((tdx != 0).sum()) < dx.numel()


def test_pool_nan_rules():
    """The header's rules on a hand-made plane: a NaN beats numbers, the last
    NaN of a window is kept, -inf everywhere selects the first tap inside the
    image, padding never wins."""
    x = torch.zeros((1, 4, 4, 8), dtype=F64)
    nan = float("nan")
    x[0, :, :, 0] = torch.tensor([[1., 2, 2, 0], [nan, 5, nan, 0], [0, 0, nan, 0], [0, 0, 0, 9]])
    x[0, :, :, 1] = -float("inf")
    dy = torch.ones((1, 2, 2, 8), dtype=torch.int64)
    y, tap, dx = S.pool_loop_ref(x, dy, (3, 2, 1))
    # window (0, 0) covers rows -1..1, cols -1..1: the NaN at pixel (1, 0) is tap 2 * 3 + 1
    assert y[0, 0, 0, 0].isnan() and tap[0, 0, 0, 0] == 7
    # window (0, 1) covers cols 1..3: 2 (tap 3), 2, 0 / 5, NaN (tap 7), 0: the NaN wins over the 5
    assert y[0, 0, 1, 0].isnan() and tap[0, 0, 1, 0] == 7
    # window (1, 0): rows 1..3, cols -1..1: the NaN at pixel (1, 0) is tap 0 * 3 + 1
    assert y[0, 1, 0, 0].isnan() and tap[0, 1, 0, 0] == 1
    # window (1, 1): rows 1..3, cols 1..3: 5, NaN (tap 1), 0 / 0, NaN (tap 4), 0 / 0, 0, 9:
    # the last NaN is kept, the 9 after it does not win
    assert y[0, 1, 1, 0].isnan() and tap[0, 1, 1, 0] == 4
    assert dx[0, 2, 2, 0] == 1 and dx[0, 1, 2, 0] == 1 and dx[0, 1, 0, 0] == 2 and dx[0, 3, 3, 0] == 0
    # all -inf: first tap inside the image ((1, 1) for the corner window, (0, 0) for the inner one)
    assert y[0, 0, 0, 1] == -float("inf") and tap[0, 0, 0, 1] == 4 and tap[0, 1, 1, 1] == 0
    # ties: zeros everywhere in channel 2: first tap inside the image
    assert tap[0, 0, 0, 2] == 4 and tap[0, 0, 1, 2] == 3 and tap[0, 1, 0, 2] == 1 and tap[0, 1, 1, 2] == 0


def test_pool_big_case_takes_a_second_grid_trip():
    ksp, shape = S.POOL_BIG
    fwd, bwd = S.pool_totals(ksp, shape)
    cap = S.POOL_MAX_BLOCKS * S.POOL_THREADS
    assert fwd > cap and bwd > cap and S.pool_grid(fwd) == S.pool_grid(bwd) == S.POOL_MAX_BLOCKS
    # and no smaller listed height does for the forward
    n, c, h, w = shape
    assert S.pool_totals(ksp, (n, c, h - 16, w))[0] <= cap
    for k2, sh in S.POOL_SMALL:
        assert max(S.pool_totals(k2, sh)) < cap
    assert (2, 2, 0) in [k for k, _ in S.POOL_SMALL]
    x, dy = S.pool_inputs((2, 2, 0), (2, 24, 6, 7), "ints")
    assert not bool(S.pool_loop_ref(x, dy, (2, 2, 0))[2][:, :, 6].any())  # the last column is in no window


# ---- bilinear resize -------------------------------------------------------------------
@pytest.mark.parametrize("n,in_hw,out_hw", S.RESIZE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_resize_reference_is_interpolate_float64(n, in_hw, out_hw):
    for c in (1, 8):
        for const in (False, True):
            x, ref = S.resize_case(n, in_hw, out_hw, c, const)
            want = F.interpolate(x.permute(0, 3, 1, 2).to(F64), size=out_hw, mode="bilinear", align_corners=False)
            got = S.resize_ref(x.to(F64), out_hw)
            assert torch.allclose(got, want.permute(0, 2, 3, 1), atol=1e-12, rtol=0)
            assert torch.equal(ref, got.to(torch.bfloat16))
            if const:
                assert torch.equal(got, x[:, :1, :1].to(F64).expand_as(got))


def test_resize_cases_reach_the_edges():
    js = set()
    for n, (ih, iw), (oh, ow) in S.RESIZE_CASES:
        for i, o in ((ih, oh), (iw, ow)):
            js.add(int(np.log2(o / i)))
            i0, i1, l0, l1 = S.resize_src(o, i)
            assert int(i1.max()) == i - 1 and int(i0.min()) == 0
    assert js == set(S.RESIZE_J)
    # r < 0 is clamped (the first output of an upscale), and i0 = in - 1 keeps i1 = i0 with l1 != 0
    i0, i1, l0, l1 = S.resize_src(12, 3)
    assert float(l1[0]) == 0.0 and 0.25 * 0.5 - 0.5 < 0
    assert int(i0[-1]) == 2 and int(i1[-1]) == 2 and float(l1[-1]) > 0
    # pixels per launch: ragged blocks and more than one
    ps = [n * oh * ow for n, _, (oh, ow) in S.RESIZE_CASES]
    assert max(ps) > 256 and any(p % 256 for p in ps) and 4608 in ps
    assert all(c % 8 for c in S.RESIZE_C_SCALAR) and not any(c % 8 for c in S.RESIZE_C_VECTOR)
