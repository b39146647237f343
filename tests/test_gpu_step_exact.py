"""Bit-exact tests of the four kernels that end a training step: cross-entropy
(loss.hip), one-launch SGD (optim.hip), the training max pool (pool_train.hip)
and the bilinear resize forward (resize.hip).  Inputs and references are
tests/_step_exact.py's, proved on the CPU by tests/test_step_exact_cpu.py.  The
library entry points are called directly on buffers with guard rows of 0xFF
bytes (tests/test_gpu_exact.py's Guarded); a few cases also go through the
Python ops.  Every comparison is torch.equal over all elements, except the
row losses of the uniform cross-entropy rows (log C is not exact: 1e-4, as
tests/test_optim.py)."""
import ctypes

import numpy as np
import pytest
import torch

import _exact as E
import _step_exact as S
from test_gpu_exact import Guarded, _ptr, _same, _stream

pytestmark = pytest.mark.gpu

BF = torch.bfloat16
F32 = torch.float32
DTYPES = {"bf16": BF, "fp32": F32}


def _sync():
    torch.cuda.synchronize()


def _bytes(t):
    return t.contiguous().view(torch.uint8).clone()


def _all_ff(t):
    return bool((t.contiguous().view(torch.uint8) == 0xFF).all())


# ---- 1. cross-entropy ------------------------------------------------------------------
@pytest.fixture(scope="module")
def loss_lib(gpu_build):
    from vgpu.ops.loss import _lib
    return _lib()


def _xent_id(v):
    family, kind, rows, c, bchw, ignore = v
    return f"{family}-{kind}-{rows}x{c}-ign{ignore}" + ("" if bchw is None else "-" + "x".join(map(str, bchw)))


def _xent_call(lib, case, lay, dtype, what):
    """Run vgpu_cross_entropy_fwd_bwd2 on guarded buffers; returns (dlogits
    storage, loss_rows, out) after the guard, pad and input checks."""
    rows, c = case.rows, case.c
    x = S.xent_store(lay, case.x, dtype, float("nan")).cuda()  # NaN in the pad columns of the parent
    x_before = _bytes(x)
    t = case.t.cuda()
    width = lay.numel // rows
    dx = Guarded(rows, width, dtype)
    need = lib.vgpu_cross_entropy_rows_workspace(rows, c)
    assert need == S.xent_workspace(rows, c), what
    lr = Guarded(1, need, F32)
    out = Guarded(1, 2, F32)
    hw, bs, ps, cs = lay.args
    rc = lib.vgpu_cross_entropy_fwd_bwd2(_ptr(x), _ptr(t), lr.ptr, out.ptr, dx.ptr, rows, c, case.ignore, hw, bs, ps,
                                         cs, int(dtype == BF), _stream())
    assert rc == 0, what
    _sync()
    assert dx.intact() and lr.intact() and out.intact(), what
    assert torch.equal(_bytes(x), x_before) and torch.equal(t.cpu(), case.t), what
    if width != c:  # padded rows: the pad keeps the sentinel, the parent its NaNs
        assert _all_ff(dx.t[:, c:]), f"{what}: the pad columns of dlogits were written"
        assert bool(x.view(rows, width)[:, c:].isnan().all())
    return dx.t.reshape(-1), lr.t.reshape(-1), out.t.reshape(-1)


def _grad_rows(store, lay, rows, c):
    """[rows, C] gathered from dlogits' storage at the layout's offsets."""
    return store[S.xent_offsets(lay, rows, c).reshape(-1).to(store.device)].view(rows, c)


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("spec", S.xent_layout_cases(), ids=_xent_id)
def test_cross_entropy_exact(loss_lib, spec, dtype):
    """Selection rows (gradient onehot(hot) - onehot(t), row loss 0 or 256 + h,
    mean and reciprocal count as numpy float32 gives them) and uniform rows
    (gradient 1 / C - onehot(t)) on every launch path, both sides of the 64 / 65
    thresholds, ragged narrow blocks, every layout; loss_rows is exactly the
    workspace the library asks for."""
    family, kind, rows, c, bchw, ignore = spec
    dt = DTYPES[dtype]
    case = S.xent_case(family, rows, c, ignore)
    lay = S.xent_layout(kind, rows, c, bchw)
    what = f"{_xent_id(spec)} {dtype}, path {S.xent_path(rows, c)}"
    store, lr, out = _xent_call(loss_lib, case, lay, dt, what)
    _same(_grad_rows(store, lay, rows, c), case.grad.to(dt), f"dlogits [row, class], {what}")
    want_out = torch.from_numpy(case.out)
    print(what, "out", out.tolist(), "want", want_out.tolist())
    if case.exact_loss:
        _same(lr[:rows], case.loss_rows.to(F32), f"loss_rows, {what}")
        _same(out, want_out, f"out = (mean, 1 / valid), {what}")
    else:
        torch.testing.assert_close(lr[:rows].cpu().double(), case.loss_rows, atol=1e-4, rtol=1e-4)
        torch.testing.assert_close(out[:1].cpu().double(), want_out[:1].double(), atol=1e-4, rtol=1e-4)
        _same(out[1:], want_out[1:], f"out[1] = 1 / valid, {what}")


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("rows,c,ignore", [(65, 65, -100), (257, 21, 5), (3, 4097, 4000)])
def test_cross_entropy_every_row_ignored(loss_lib, rows, c, ignore, dtype):
    """No valid row: the gradient is all zeros, out[1] is 0 and the mean is 0 / 0."""
    dt = DTYPES[dtype]
    case = S.xent_case("selection", rows, c, ignore, 0)
    lay = S.xent_layout("dense", rows, c)
    store, lr, out = _xent_call(loss_lib, case, lay, dt, f"all ignored {rows}x{c}")
    _same(store.view(rows, c), torch.zeros((rows, c), dtype=dt), "dlogits")
    _same(lr[:rows], torch.zeros(rows, dtype=F32), "loss_rows")
    out = out.cpu()
    assert float(out[1]) == 0.0 and bool(out[0].isnan()), out


@pytest.mark.parametrize("dtype", list(DTYPES))
@pytest.mark.parametrize("kind,rows,c,bchw", S.xent_op_cases(), ids=lambda v: str(v).replace(" ", ""))
def test_cross_entropy_op_exact(gpu_build, kind, rows, c, bchw, dtype):
    """vgpu.ops.loss.cross_entropy with 8 valid rows and (loss * 4).backward():
    the gradient is 4 / 8 * (onehot(hot) - onehot(t)) with the logits' strides.
    A padded-row view gets it through its parent, whose gradient is zero
    outside the view.  (Autograd repacks what it keeps for a non-dense tensor,
    so the strides are read off the gradient as the backward hands it over.)"""
    from vgpu.ops.loss import cross_entropy
    dt = DTYPES[dtype]
    case = S.xent_case("selection", rows, c, -100, 8)
    lay = S.xent_layout(kind, rows, c, bchw)
    parent = S.xent_store(lay, case.x, dt, 0.0).cuda().requires_grad_()
    x = S.xent_tensor(lay, parent)  # a view of the leaf: dense, channels-last, NCHW or padded rows
    assert x.stride() == lay.stride
    handed = []
    x.register_hook(handed.append)
    tshape = (rows,) if bchw is None else (bchw[0], bchw[2], bchw[3])
    loss = cross_entropy(x, case.t.view(tshape).cuda())
    (loss * 4).backward()
    _sync()
    want_loss = np.float32(float(case.loss_rows.sum())) / np.float32(8)
    got_loss = float(loss.detach())
    assert loss.dtype == F32 and got_loss == float(want_loss), (got_loss, want_loss)
    (g,) = handed
    assert g.stride() == x.stride() and g.dtype == dt and g.shape == x.shape
    g_rows = g if bchw is None else g.permute(0, 2, 3, 1).reshape(rows, c)
    _same(g_rows.contiguous(), (case.grad * 0.5).to(dt), f"x.grad [row, class], {kind}")
    # through the view into the leaf: the same values at the layout's offsets, zero in the pad
    _same(parent.grad, S.xent_store(lay, case.grad * 0.5, dt, 0.0), f"parent.grad storage, {kind}")


# ---- 2. SGD ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sgd_lib(gpu_build):
    from vgpu.ops.optim import _lib
    return _lib()


def _sgd_launch(lib, ps, gs, ms, ns, hp, first, nseg=None):
    k = len(ps)
    arr = ctypes.c_void_p * max(k, 1)
    return lib.vgpu_sgd_bf16(arr(*ps), arr(*gs), arr(*ms), (ctypes.c_int64 * max(k, 1))(*ns), k if nseg is None else nseg,
                             hp["lr"], hp["momentum"], hp["dampening"], hp["weight_decay"], int(hp["nesterov"]),
                             int(first), _stream())


def _gbuf(n, fill=None):
    return Guarded(1, n, BF, None if fill is None else fill.to(BF).view(1, n))


@pytest.mark.parametrize("hp", list(S.SGD_HP))
@pytest.mark.parametrize("name", list(S.SGD_SIZES))
def test_sgd_direct_exact(sgd_lib, name, hp):
    """vgpu_sgd_bf16 over the segment tables of S.SGD_SIZES: a first step (the
    momentum buffers hold 0xFF NaNs and must not be read), two continuing
    steps with fresh gradients, and a continuing step from integer momentum.
    p, g and m of every segment sit in guarded buffers of their own; g must
    come back unchanged."""
    kw = S.SGD_HP[hp]
    segs = S.sgd_case(name)
    ns = [p0.numel() for p0, _, _ in segs]
    P = [_gbuf(n, p0) for n, (p0, _, _) in zip(ns, segs)]
    M = [_gbuf(n) for n in ns]  # poisoned
    assert all(bool(m.t.isnan().all()) for m in M)
    refs = [S.sgd_run_ref(p0, gs, kw) for p0, _, gs in segs]
    for step in range(S.SGD_STEPS):
        G = [_gbuf(n, gs[step]) for n, (_, _, gs) in zip(ns, segs)]
        rc = _sgd_launch(sgd_lib, [b.t.data_ptr() for b in P], [b.t.data_ptr() for b in G],
                         [b.t.data_ptr() for b in M], ns, kw, step == 0)
        assert rc == 0
        _sync()
        for i, (n, (_, _, gs)) in enumerate(zip(ns, segs)):
            what = f"{name}/{hp} step {step + 1}, segment {i} of {n} (first block {S.sgd_blocks(ns)[i]})"
            assert P[i].intact() and G[i].intact() and M[i].intact(), what
            _same(G[i].t.view(-1), gs[step].to(BF), f"g, {what}")
            _same(P[i].t.view(-1), refs[i][step][0].to(BF), f"p, {what}")
            _same(M[i].t.view(-1), refs[i][step][1].to(BF), f"m, {what}")
    # a continuing step from integer momentum
    P = [_gbuf(n, p0) for n, (p0, _, _) in zip(ns, segs)]
    M = [_gbuf(n, m0) for n, (_, m0, _) in zip(ns, segs)]
    G = [_gbuf(n, gs[0]) for n, (_, _, gs) in zip(ns, segs)]
    rc = _sgd_launch(sgd_lib, [b.t.data_ptr() for b in P], [b.t.data_ptr() for b in G], [b.t.data_ptr() for b in M],
                     ns, kw, False)
    assert rc == 0
    _sync()
    for i, (p0, m0, gs) in enumerate(segs):
        (pr, mr), = S.sgd_run_ref(p0, gs[:1], kw, m0)
        assert P[i].intact() and G[i].intact() and M[i].intact()
        _same(P[i].t.view(-1), pr.to(BF), f"p, continuing from integers, segment {i}")
        _same(M[i].t.view(-1), mr.to(BF), f"m, continuing from integers, segment {i}")


def test_sgd_refusals_write_nothing(sgd_lib):
    """nseg 0 and 49, n = 12 and a pointer offset by 2 bytes return -1 and
    leave every buffer byte-identical."""
    kw = S.SGD_HP["wd"]
    g = E.gen(7)
    n = 16
    bufs = [[_gbuf(n, E.nonzero_ints((n,), g, 4)) for _ in range(49)] for _ in range(3)]
    before = [[_bytes(b.raw) for b in kind] for kind in bufs]
    ptrs = [[b.t.data_ptr() for b in kind] for kind in bufs]

    def call(k, ns, nseg=None, shift=(0, 0, 0)):
        return _sgd_launch(sgd_lib, [p + shift[0] for p in ptrs[0][:k]], [p + shift[1] for p in ptrs[1][:k]],
                           [p + shift[2] for p in ptrs[2][:k]], ns, kw, False, nseg)

    assert call(1, [n], nseg=0) == -1
    assert call(49, [n] * 49) == -1
    assert call(2, [n, 12]) == -1
    assert call(1, [12]) == -1
    for which in range(3):
        shift = [0, 0, 0]
        shift[which] = 2
        assert call(2, [8, 8], shift=tuple(shift)) == -1
    _sync()
    for kind, kb in zip(bufs, before):
        for b, was in zip(kind, kb):
            assert torch.equal(_bytes(b.raw), was)
    assert call(48, [n] * 48) == 0  # and the largest table it takes
    _sync()
    assert all(b.intact() for kind in bufs for b in kind)
    assert torch.equal(_bytes(bufs[0][48].raw), before[0][48])


@pytest.mark.parametrize("hp", list(S.SGD_CLASS_RUNS))
def test_sgd_class_exact(gpu_build, hp):
    """vgpu.ops.optim.SGD over 50 tensors the native path takes (one of them
    channels-last) and one it does not: the native entry gets 48 and then 2
    tensors per step, and all 51 results equal the reference."""
    import vgpu.ops.optim as O
    steps = S.SGD_CLASS_RUNS[hp]
    kw = S.SGD_HP[hp]
    data = S.sgd_class_case(steps)

    def dev(t, shape):
        t = t.to(BF).cuda()
        return t.contiguous(memory_format=E.CL) if len(shape) == 4 else t

    params = [torch.nn.Parameter(dev(p0, sh)) for (p0, _), sh in zip(data, S.SGD_CLASS_SHAPES)]
    assert params[0].is_contiguous(memory_format=E.CL) and not params[0].is_contiguous()
    opt = O.SGD(params, **kw)
    calls, launches = [], []
    lib = O._lib()

    class Spy:  # the library with vgpu_sgd_bf16's segment count recorded
        vgpu_sgd_max_segments = staticmethod(lib.vgpu_sgd_max_segments)

        @staticmethod
        def vgpu_sgd_bf16(p, g, m, n, k, *rest):
            launches.append(k)
            return lib.vgpu_sgd_bf16(p, g, m, n, k, *rest)

    orig, orig_lib = O.sgd_bf16_, O._lib
    O.sgd_bf16_ = lambda *a, **k: (calls.append(len(a[0])), orig(*a, **k))[1]
    O._lib = lambda: Spy
    try:
        for step in range(steps):
            for p, (_, gs), sh in zip(params, data, S.SGD_CLASS_SHAPES):
                p.grad = dev(gs[step], sh)
            opt.step()
    finally:
        O.sgd_bf16_, O._lib = orig, orig_lib
    _sync()
    assert calls == [50] * steps, calls  # the 50 eligible tensors of a step, natively ...
    assert launches == [48, 2] * steps, launches  # ... in two launches of the library entry
    for i, (p, (p0, gs)) in enumerate(zip(params, data)):
        pr, mr = S.sgd_run_ref(p0, gs, kw)[-1]
        _same(p.detach(), pr.to(BF), f"p of tensor {i} {tuple(p.shape)}, {hp}")
        _same(opt.state[p]["momentum_buffer"], mr.to(BF), f"m of tensor {i} {tuple(p.shape)}, {hp}")


# ---- 3. training max pool --------------------------------------------------------------
@pytest.fixture(scope="module")
def pool_lib(gpu_build):
    from vgpu.native import load_kernels
    return load_kernels()


def _nan_same(got, ref, what):
    """_same where a NaN equals a NaN: the same places hold one, and the rest is equal."""
    ref = ref.to(got.device)
    assert torch.equal(got.isnan(), ref.isnan()), f"{what}: NaNs at different places"
    _same(torch.where(got.isnan(), 77.0, got), torch.where(ref.isnan(), 77.0, ref), what)


def _pool_run(lib, x, dy, ksp, shape, ref, what):
    """All three entry points on guarded buffers against ref = (y, tap, dx),
    [N, ., ., C] tensors of the kernels' types."""
    k, s, p = ksp
    n, c, h, w = shape
    oh, ow = E.out_hw(h, w, k, s, p)
    y_ref, tap_ref, dx_ref = ref
    xd, dyd = x.cuda().contiguous(), dy.cuda().contiguous()
    x_before = _bytes(xd) if xd.numel() < 1 << 20 else None
    y, idx = Guarded(n * oh * ow, c), Guarded(n * oh * ow, c, torch.uint8)
    rc = lib.vgpu_maxpool_fwd_idx_nhwc(_ptr(xd), y.ptr, idx.ptr, n, h, w, c, k, s, p, _stream())
    assert rc == 0, what
    _sync()
    assert y.intact() and idx.intact(), what
    _nan_same(y.t.view(n, oh, ow, c), y_ref, f"y, {what}")
    _same(idx.t.view(n, oh, ow, c), tap_ref, f"idx bytes, {what}")
    # the NCHW-output entry: the same taps, y permuted
    y2, idx2 = Guarded(n * c, oh * ow), Guarded(n * oh * ow, c, torch.uint8)
    rc = lib.vgpu_maxpool_fwd_idx_nchw_out(_ptr(xd), y2.ptr, idx2.ptr, n, h, w, c, k, s, p, _stream())
    assert rc == 0, what
    _sync()
    assert y2.intact() and idx2.intact(), what
    _nan_same(y2.t.view(n, c, oh, ow), y_ref.permute(0, 3, 1, 2).contiguous(), f"y of nchw_out, {what}")
    _same(idx2.t.view(n, oh, ow, c), tap_ref, f"idx bytes of nchw_out, {what}")
    # the gather backward from the kernel's own idx
    dx = Guarded(n * h * w, c)
    rc = lib.vgpu_maxpool_bwd_nhwc(_ptr(dyd), idx.ptr, dx.ptr, n, h, w, c, k, s, p, _stream())
    assert rc == 0, what
    _sync()
    assert dx.intact() and idx.intact(), what
    _same(dx.t.view(n, h, w, c), dx_ref, f"dx, {what}")
    if x_before is not None:
        assert torch.equal(_bytes(xd), x_before), what


@pytest.mark.parametrize("kind", S.POOL_KINDS)
@pytest.mark.parametrize("ksp,shape", S.POOL_SMALL, ids=lambda v: "x".join(map(str, v)))
def test_maxpool_train_exact(pool_lib, ksp, shape, kind):
    """y, the tap bytes and dx against the plain loop: constant planes (every
    window a full tie), integers in [-3, 3], and the same with NaNs and an
    all -inf plane."""
    x, dy = S.pool_inputs(ksp, shape, kind)
    y, tap, dx = S.pool_loop_ref(x, dy, ksp)
    _pool_run(pool_lib, x.to(BF), dy.to(BF), ksp, shape, (y.to(BF), tap, dx.to(BF)), f"{ksp} on {shape}, {kind}")


def test_maxpool_train_grid_stride_exact(pool_lib):
    """(3, 2, 1) on (2, 64, 512, 520): both kernels' grids are capped at 4096
    blocks and their grid-stride loops take a second trip."""
    ksp, shape = S.POOL_BIG
    fwd, bwd = S.pool_totals(ksp, shape)
    assert min(fwd, bwd) > S.POOL_MAX_BLOCKS * S.POOL_THREADS
    x, dy, y, tap, dx = S.pool_big_case()
    _pool_run(pool_lib, x, dy, ksp, shape, (y, tap, dx), f"{ksp} on {shape}")


def test_maxpool_train_refusals_write_nothing(pool_lib):
    """C = 12 and 2 * pad > k return -1 from all three entry points and write nothing."""
    n, h, w = 1, 6, 6
    for c, (k, s, p) in ((12, (3, 2, 1)), (8, (3, 2, 2)), (8, (16, 1, 0))):
        x = torch.ones((n * h * w, c), dtype=BF, device="cuda")
        bufs = [Guarded(n * h * w, c), Guarded(n * h * w, c, torch.uint8), Guarded(n * h * w, c)]
        y, idx, dx = bufs
        st = _stream()
        assert pool_lib.vgpu_maxpool_fwd_idx_nhwc(_ptr(x), y.ptr, idx.ptr, n, h, w, c, k, s, p, st) == -1
        assert pool_lib.vgpu_maxpool_fwd_idx_nchw_out(_ptr(x), y.ptr, idx.ptr, n, h, w, c, k, s, p, st) == -1
        assert pool_lib.vgpu_maxpool_bwd_nhwc(_ptr(x), idx.ptr, dx.ptr, n, h, w, c, k, s, p, st) == -1
        _sync()
        assert all(_all_ff(b.raw) for b in bufs), (c, k, s, p)


# ---- 4. bilinear resize ----------------------------------------------------------------
@pytest.fixture(scope="module")
def resize_lib(gpu_build):
    from vgpu.ops import interp
    x = torch.zeros((1, 8, 2, 2), dtype=BF, device="cuda").contiguous(memory_format=E.CL)
    interp._forward(x, (2, 2), native=True)  # binds the entry point's argtypes
    from vgpu.native import load_kernels
    return load_kernels()


def _resize_run(lib, x, ref, n, in_hw, out_hw, c, shift_x=0, shift_y=0):
    """vgpu_resize_bilinear_nhwc with x and / or y starting `shift` elements
    into their buffers (a misaligned pointer takes the scalar path)."""
    P = n * out_hw[0] * out_hw[1]
    xin = torch.full((x.numel() + 8,), float("nan"), dtype=BF, device="cuda")
    xin[shift_x:shift_x + x.numel()] = x.to(BF).reshape(-1).cuda()
    y = Guarded(P + 1, c)
    flat = y.t.view(-1)
    xp = ctypes.c_void_p(xin.data_ptr() + 2 * shift_x)
    yp = ctypes.c_void_p(y.t.data_ptr() + 2 * shift_y)
    vec = c % 8 == 0 and xp.value % 16 == 0 and yp.value % 16 == 0
    what = f"{in_hw} -> {out_hw}, N {n}, C {c}, x + {shift_x}, y + {shift_y}, {'vector' if vec else 'scalar'} path"
    rc = lib.vgpu_resize_bilinear_nhwc(xp, yp, n, in_hw[0], in_hw[1], c, out_hw[0], out_hw[1], _stream())
    assert rc == 0, what
    _sync()
    assert y.intact(), what
    assert _all_ff(flat[:shift_y]) and _all_ff(flat[shift_y + P * c:]), f"{what}: written outside y"
    _same(flat[shift_y:shift_y + P * c].view(n, *out_hw, c), ref, f"y, {what}")
    return vec


@pytest.mark.parametrize("n,in_hw,out_hw", S.RESIZE_CASES, ids=lambda v: str(v).replace(" ", ""))
def test_resize_forward_exact(resize_lib, n, in_hw, out_hw):
    """Power-of-two scales on integers: the clamped first (r < 0) and last
    (i0 = in - 1) source pixels, C on the scalar (1, 21, 30) and vector (8, 24)
    paths, C = 24 through a pointer that is off by one element, and two
    images holding different constants."""
    for c in S.RESIZE_C_SCALAR + S.RESIZE_C_VECTOR:
        x, ref = S.resize_case(n, in_hw, out_hw, c)
        assert _resize_run(resize_lib, x, ref, n, in_hw, out_hw, c) == (c in S.RESIZE_C_VECTOR)
    x, ref = S.resize_case(n, in_hw, out_hw, 24)
    assert not _resize_run(resize_lib, x, ref, n, in_hw, out_hw, 24, shift_x=1)
    assert not _resize_run(resize_lib, x, ref, n, in_hw, out_hw, 24, shift_y=1)
    assert not _resize_run(resize_lib, x, ref, n, in_hw, out_hw, 24, shift_x=1, shift_y=1)
    if n == 2:  # image 1 must read nothing of image 0
        for c in (21, 8):
            x, ref = S.resize_case(n, in_hw, out_hw, c, True)
            assert bool((ref[1] == -5).all()) and bool((ref[0] == 7).all())
            _resize_run(resize_lib, x, ref, n, in_hw, out_hw, c)


@pytest.mark.parametrize("c", [8, 21])
def test_resize_op_exact(gpu_build, c):
    """vgpu.ops.interp._forward(x, size, native=True): a vector and a scalar case."""
    from vgpu.ops import interp
    n, in_hw, out_hw = 2, (24, 24), (48, 48)
    x, ref = S.resize_case(n, in_hw, out_hw, c)
    xd = x.to(BF).permute(0, 3, 1, 2).cuda().contiguous(memory_format=E.CL)
    y = interp._forward(xd, out_hw, native=True)
    _sync()
    assert y.shape == (n, c, *out_hw) and y.is_contiguous(memory_format=E.CL)
    _same(y.permute(0, 2, 3, 1).contiguous(), ref, f"y through the op, C {c}")
