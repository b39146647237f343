"""Exact-integer tests of the BatchNorm kernels (native/kernels/bn_nhwc.hip):
every plan of plain_kind(M, C), both tuning instantiations, null parameters,
the two entry points that take their statistics as partials, and the
statistics the convolution epilogues form (conv_gemm.hip, vgpu_conv2d_nhwc_bn).

The C entry points are called directly (load_kernels()), so that eps,
momentum, the saved statistics and the partials are the test's to choose.
Outputs go into buffers with guard rows of 0xFF bytes; the fp32 workspace
starts as NaNs and has guard rows too, so a partial nobody wrote poisons the
statistics and a write past vgpu_bn_workspace(M, C) shows.

Forward on the plain path: saved mean / invstd within 1 fp32 ulp of the value
computed from int64 sums (tests/test_bn_exact_cpu.py proves that losing or
doubling one row moves them by >= 16), y within bf16's half-ulp plus eight
fp32 half-ulps of its terms.  Backward and the *_partials entry points: the
saved statistics are inputs, so d-gamma, d-beta (and, with synthetic partials,
mean, invstd, the folded coefficients and y) must EQUAL the reference.
Inputs, references and the plan mirror are tests/_bn_exact.py's."""
import ctypes
import dataclasses
import gc

import pytest
import torch

import _bn_exact as B
from _exact import round_to
from test_gpu_exact import Guarded, _ptr, _same, _stream

pytestmark = pytest.mark.gpu

BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64


@pytest.fixture(scope="module")
def lib(gpu_build):
    from vgpu.native import load_kernels
    lib = load_kernels()
    lib.vgpu_bn_act_fwd_train_add.restype = ctypes.c_int
    return lib


@pytest.fixture(scope="module", autouse=True)
def _release_memory():
    """The suite goes on in this process to tests that measure free HBM and pin
    64 GiB of host memory: hand back the cached cases and torch's cached blocks."""
    yield
    for cached in (B.fwd_partials_case, B.bwd_partials_case, B.conv_case):
        cached.cache_clear()
    gc.collect()
    torch.cuda.empty_cache()


class Switches:
    """vgpu_bn_set_fuse_small / vgpu_bn_set_tuning for one case, restored on exit."""

    def __init__(self, lib, fuse=-1, tuning=(0, 0)):
        self.lib, self.fuse, self.tuning = lib, fuse, tuning

    def __enter__(self):
        self.lib.vgpu_bn_set_fuse_small(self.fuse)
        self.lib.vgpu_bn_set_tuning(*self.tuning)

    def __exit__(self, *exc):
        self.lib.vgpu_bn_set_fuse_small(-1)
        self.lib.vgpu_bn_set_tuning(0, 0)


def _dev(t, dtype):
    return None if t is None else t.to(dtype).cuda().contiguous()


def _workspace(lib, p):
    """The NaN-filled, guarded workspace, sized by the library under the case's
    switches (which must be set) and held against the plan mirror."""
    need = lib.vgpu_bn_workspace(p.M, p.C)
    assert need == B.workspace(p.M, p.C, p.fuse != 0, p.tuning), (need, p.plan)
    ws = Guarded(need // p.C, p.C, F32)
    assert bool(ws.t.isnan().all())
    return ws


def _partials_written(ws, p):
    """Every reduction block left its pair (kind 0 and 1); the one-launch kernels leave the workspace alone."""
    G = p.plan["G"]
    part = ws.t.view(-1)[:2 * G * p.C]
    if p.plan["kind"] == 2:
        assert bool(ws.t.isnan().all()), "the one-launch plan wrote to the workspace"
    else:
        assert not bool(part.isnan().any()), f"{int(part.isnan().sum())} partial sums unwritten, {p.plan}"


def _within(got, ref, bound, what):
    """|got - ref| <= bound everywhere; says where the worst miss is."""
    err = (got.double().cpu() - ref).abs()
    bad = ~(err <= bound)  # a NaN misses
    if bool(bad.any()):
        over = torch.where(bad & ~err.isnan(), err / bound.clamp(min=1e-300), torch.zeros_like(err))
        at = divmod(int((over + bad).flatten().argmax()), err.shape[1])
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.numel()} out of bound; worst at {at}: got "
                             f"{got[at].item()} want {ref[at].item()} +- {bound[at].item():.3g}; first at "
                             f"{bad.nonzero()[0].tolist()}, last at {bad.nonzero()[-1].tolist()}")


def _ulp1(got, ref64, what):
    """fp32 got within 1 ulp of the fp64 reference rounded once."""
    d = B.ulps(got, ref64.float())
    print(f"{what}: max {int(d.max())} ulp")
    at = int(d.argmax())
    assert int(d.max()) <= 1, f"{what}: {int((d > 1).sum())} of {d.numel()} off by more than 1 ulp; worst " \
                              f"{int(d.max())} at {at}: got {got.flatten()[at].item()!r} want {ref64.flatten()[at].item()!r}"


def _bf16_of(got, ref32, what):
    """A bf16 parameter: the fp32 value rounded once (either neighbour where it is within 1 ulp of a tie)."""
    ok = (B.bf16_choices(ref32.cpu()) == got.cpu().unsqueeze(0)).any(0)
    if not bool(ok.all()):
        raise AssertionError(f"{what}: {int((~ok).sum())} of {ok.numel()} are not the fp32 value rounded to bf16; "
                             f"first at {int((~ok).nonzero()[0])}")


# ---- Part A: the plain-path forward ---------------------------------------------------
def _run_forward(lib, p, x, add=None, mom=0.25):
    """One forward of case p through its entry point.  -> dict of the outputs (device tensors / Guarded)."""
    pdt = BF if p.bf16 else F32
    gamma, beta, rm_old, rv_old = B.fwd_params(p.C)
    if not p.affine:
        gamma = beta = None
    with Switches(lib, p.fuse, p.tuning):
        ws = _workspace(lib, p)
        xd = _dev(x, BF)
        y = Guarded(p.M, p.C)
        g, b = _dev(gamma, pdt), _dev(beta, pdt)
        rm = Guarded(1, p.C, pdt, fill=rm_old.to(pdt)) if p.running else None
        rv = Guarded(1, p.C, pdt, fill=rv_old.to(pdt)) if p.running else None
        rmp, rvp = (rm.ptr, rv.ptr) if p.running else (None, None)
        tail = (p.M, p.C, B.EPS, mom, B.ACT[p.act], int(p.bf16))
        coef = None
        if p.entry == "coef":
            coef = Guarded(4, p.C, F32)
            rc = lib.vgpu_bn_act_fwd_train_coef(_ptr(xd), y.ptr, _ptr(g), _ptr(b), rmp, rvp, coef.ptr, ws.ptr, *tail,
                                                _stream())
            mean, invstd = coef.t[2], coef.t[3]
            stat_bufs = [coef]
        else:
            mean, invstd = Guarded(1, p.C, F32), Guarded(1, p.C, F32)
            stat_bufs = [mean, invstd]
            if p.entry == "add":
                addd = _dev(add, BF)
                rc = lib.vgpu_bn_act_fwd_train_add(_ptr(xd), y.ptr, _ptr(g), _ptr(b), rmp, rvp, mean.ptr, invstd.ptr,
                                                   ws.ptr, *tail, _ptr(addd), _stream())
            else:
                rc = lib.vgpu_bn_act_fwd_train(_ptr(xd), y.ptr, _ptr(g), _ptr(b), rmp, rvp, mean.ptr, invstd.ptr,
                                               ws.ptr, *tail, _stream())
            mean, invstd = mean.t[0], invstd.t[0]
        torch.cuda.synchronize()
    assert rc == 0, rc
    for buf in [y, ws, *stat_bufs] + ([rm, rv] if p.running else []):
        assert buf.intact(), "a guard row was written"
    _partials_written(ws, p)
    return dict(y=y.t, mean=mean, invstd=invstd, coef=None if coef is None else coef.t, mom=mom,
                rm=rm.t[0] if p.running else None, rv=rv.t[0] if p.running else None,
                gamma=gamma, beta=beta, rm_old=rm_old, rv_old=rv_old)


def _check_forward(p, x, out, add, what):
    st = B.fwd_stats(x)
    mean, invstd = out["mean"].cpu(), out["invstd"].cpu()
    # saved statistics: 1 ulp of the once-rounded exact value; an integer mean is met exactly
    _ulp1(mean, st.mean, f"{what} mean")
    _ulp1(invstd, st.invstd, f"{what} invstd")
    _same(mean[st.mean_exact], st.mean.float()[st.mean_exact], f"{what} mean where it is an integer")
    gamma, beta = out["gamma"], out["beta"]
    if out["coef"] is not None:
        # rows 2 / 3 of coef ARE the saved statistics here; rows 0 / 1 are s and t formed from them in fp32
        coef = out["coef"].cpu()
        g32 = torch.ones(p.C) if gamma is None else gamma.float()
        b32 = torch.zeros(p.C) if beta is None else beta.float()
        s32 = g32 * invstd
        _same(coef[0], s32, f"{what} coef s = gamma * invstd")
        t64 = b32.double() - mean.double() * s32.double()   # exact in fp64 (24 + 24 bits); the kernel rounds once
        d = B.ulps(coef[1], t64.float())                     # (fma) or twice (mul, then sub): 1 ulp of the larger term
        big = torch.maximum(b32.abs(), (mean * s32).abs())
        err = (coef[1].double() - t64).abs()
        assert bool(((d <= 1) | (err <= 2.0 ** -23 * big.double())).all()), f"{what} coef t = beta - mean * s"
    if p.running:
        mom = out["mom"]
        pdt = BF if p.bf16 else F32
        rm, rv = out["rm"].cpu(), out["rv"].cpu()
        assert rm.dtype == pdt and rv.dtype == pdt
        # (1 - m) * old and m * mean are exact (m = 0.25 or 1, |old| a multiple of 4): one rounding of their sum
        rm32 = ((1 - mom) * out["rm_old"] + mom * mean.double()).float()
        rv32_exact = ((1 - mom) * out["rv_old"] + mom * st.unbiased)
        if p.bf16:
            _same(rm, rm32.to(BF), f"{what} running mean from the saved mean, momentum {mom}")
            if mom == 1.0:
                _bf16_of(rv, rv32_exact.float(), f"{what} running var, momentum 1")
        else:
            _same(rm, rm32, f"{what} running mean from the saved mean, momentum {mom}")
            _ulp1(rm, (1 - mom) * out["rm_old"] + mom * st.mean, f"{what} running mean, momentum {mom}")
            if mom == 1.0:
                _ulp1(rv, rv32_exact, f"{what} running var, momentum 1")
        if mom != 1.0:  # (1 - m) * 3 is exact; m * unbiased and the sum each round: 2 ulp of fp32, a step of bf16
            if p.bf16:
                assert bool(((rv.double() - rv32_exact).abs() <= 2.0 ** -7 * rv32_exact.abs()).all())
            else:
                assert int(B.ulps(rv, rv32_exact.float()).max()) <= 2, f"{what} running var, momentum {mom}"
    z, delta = B.fwd_ref(x, st, gamma, beta, p.act, add)
    _within(out["y"], z, B.y_bound(z, delta), f"{what} y [row, channel]")


def _add_for(p):
    return torch.randint(-8, 9, (p.M, p.C), generator=B.gen(p.M + p.C)) if p.entry == "add" else None


@pytest.mark.parametrize("p", B.PLAIN, ids=lambda p: p.id)
def test_bn_forward_dense_exact_statistics(lib, p):
    """Dense integers (no row equal to row 0, one constant channel): saved mean and
    invstd within 1 ulp, running statistics, coef, y within bf16's half-ulp, on
    every plan; M = 1 included."""
    x = B.fwd_input(p.M, p.C, "dense")
    add = _add_for(p)
    for mom in (0.25, 1.0) if p.running else (0.25,):
        out = _run_forward(lib, p, x, add, mom)
        _check_forward(p, x, out, add, f"momentum {mom}, {p.what}, {p.plan}")
    if p.entry == "coef":  # rows 2 / 3 of coef are what the plain entry saves, bit for bit; y too
        plain = _run_forward(lib, dataclasses.replace(p, entry="train"), x, None, mom)
        _same(out["mean"], plain["mean"], "coef's mean against vgpu_bn_act_fwd_train's")
        _same(out["invstd"], plain["invstd"], "coef's invstd against vgpu_bn_act_fwd_train's")
        _same(out["y"], plain["y"], "y of the coef entry against vgpu_bn_act_fwd_train's")
    cc = B.const_channel(p.C)   # variance exactly 0: invstd = 1 / sqrt(eps), whatever the clamp had to do
    _ulp1(out["invstd"][cc:cc + 1].cpu(), torch.tensor([1.0 / B.EPS ** 0.5], dtype=F64), "constant channel invstd")


@pytest.mark.parametrize("p", B.SINGLE, ids=lambda p: p.id)
def test_bn_forward_single_row_at_plan_edges(lib, p):
    """Every row equals row 0 but one, placed at each edge the plan has (the
    first / last row, each side of a block, of an unrolled step, of a fused row
    range, of a thread's row stride): that row is counted once, in its place."""
    add = _add_for(p)
    for r in B.edge_rows(p.M, p.C, p.fuse != 0, p.tuning):
        x = B.fwd_input(p.M, p.C, "single", r)
        out = _run_forward(lib, p, x, add)
        _check_forward(p, x, out, add, f"row {r} of {p.what}, {p.plan}")


@pytest.mark.parametrize("p", B.NO_ADD, ids=lambda p: p.id)
def test_bn_forward_add_refused_on_three_pass_shapes(lib, p):
    """The three-launch plan has no add form: -2, and nothing written."""
    x = _dev(B.fwd_input(p.M, p.C, "dense"), BF)
    with Switches(lib, p.fuse, p.tuning):
        ws = _workspace(lib, p)
        y, mean, invstd = Guarded(p.M, p.C), Guarded(1, p.C, F32), Guarded(1, p.C, F32)
        rm, rv = Guarded(1, p.C, F32), Guarded(1, p.C, F32)
        rc = lib.vgpu_bn_act_fwd_train_add(_ptr(x), y.ptr, None, None, rm.ptr, rv.ptr, mean.ptr, invstd.ptr, ws.ptr,
                                           p.M, p.C, B.EPS, 0.25, 1, 0, _ptr(x), _stream())
        torch.cuda.synchronize()
    assert rc == -2
    for buf in (ws, y, mean, invstd, rm, rv):
        assert bool((buf.raw == 0xFF).all())


# ---- Part B: backward -----------------------------------------------------------------
def _run_backward(lib, p, c, act, with_add, null_grads):
    pdt = BF if p.bf16 else F32
    with Switches(lib, p.fuse, p.tuning):
        ws = _workspace(lib, p)
        xd, dyd, addd = _dev(c.x, BF), _dev(c.dy, BF), _dev(c.add, BF) if with_add else None
        g, b = _dev(c.gamma, pdt), _dev(c.beta, pdt)
        mean, invstd = _dev(c.mean, F32), _dev(c.invstd, F32)
        dx = Guarded(p.M, p.C)
        dg = None if null_grads else Guarded(1, p.C, pdt)
        db = None if null_grads else Guarded(1, p.C, pdt)
        args = (_ptr(dyd), _ptr(xd), dx.ptr, _ptr(g), _ptr(b), _ptr(mean), _ptr(invstd), dg and dg.ptr, db and db.ptr,
                ws.ptr, p.M, p.C, B.ACT[act], int(p.bf16))
        if with_add:
            rc = lib.vgpu_bn_act_bwd_add(*args, _ptr(addd), _stream())
        else:
            rc = lib.vgpu_bn_act_bwd(*args, _stream())
        torch.cuda.synchronize()
    assert rc == 0, rc
    for buf in (dx, ws) + (() if null_grads else (dg, db)):
        assert buf.intact(), "a guard row was written"
    _partials_written(ws, p)
    return dx.t, None if null_grads else dg.t[0], None if null_grads else db.t[0]


def _check_backward(lib, p, c, act, with_add, null_grads, what):
    pdt = BF if p.bf16 else F32
    dx, dg, db = _run_backward(lib, p, c, act, with_add, null_grads)
    rdg, rdb, rdx, bound, _ = B.bwd_ref(c, act, with_add)
    if not null_grads:
        _same(db, round_to(rdb, pdt), f"{what} dbeta")
        _same(dg, round_to(rdg, pdt), f"{what} dgamma")
    _within(dx, rdx, bound, f"{what} dx [row, channel]")


@pytest.mark.parametrize("p", [p for p in B.PLAIN if p.M > 1], ids=lambda p: p.id)
def test_bn_backward_dense_exact_sums(lib, p):
    """Chosen integer mean, invstd in {1, 1/2, 1/4}, gamma a power of two: z, the
    mask (rows planted at z == 0 and z == 6), dz and x-hat are exact, so d-beta
    and d-gamma EQUAL the int64 sums; dx within bf16's half-ulp.  Every
    activation; the case's own one also with add and with null d-gamma / d-beta."""
    c = B.bwd_case(p.M, p.C, "dense", affine=p.affine)
    what = f"{p.what}, {p.plan}"
    for act in B.ACT:
        _check_backward(lib, p, c, act, False, False, f"{act}, {what}")
    _check_backward(lib, p, c, p.act, True, False, f"{p.act} + add, {what}")
    _check_backward(lib, p, c, p.act, p.entry == "add", True, f"{p.act}, null grads, {what}")


@pytest.mark.parametrize("p", B.SINGLE, ids=lambda p: p.id)
def test_bn_backward_single_row_at_plan_edges(lib, p):
    """dy is zero but in one row, placed at the plan's edges."""
    for r in B.edge_rows(p.M, p.C, p.fuse != 0, p.tuning, backward=True):
        c = B.bwd_case(p.M, p.C, "single", r, affine=p.affine)
        _check_backward(lib, p, c, p.act, False, False, f"row {r}, {p.act}, {p.what}, {p.plan}")


# ---- Part B: statistics given as partials ---------------------------------------------
@pytest.mark.parametrize("q", B.PARTIALS, ids=lambda q: q.id)
def test_bn_forward_from_partials_exact(lib, q):
    """vgpu_bn_act_fwd_partials on synthetic integer pairs (every group non-zero,
    eps = 0): mean, invstd, s, t, y and the running mean at momentum 0.25 EQUAL
    the reference; the running variance at momentum 1 is within 1 ulp.  Fused
    up to G = 160 at C % 64 == 0, else the 128-group finalize tree."""
    f = B.fwd_partials_case(q.M, q.C)
    pdt = BF if q.bf16 else F32
    part = f["partial"].float().cuda().contiguous()
    x = _dev(f["x"], BF)
    g, b = _dev(f["gamma"], pdt), _dev(f["beta"], pdt)
    got = {}
    for mom in (0.25, 1.0):
        y, coef = Guarded(q.M, q.C), Guarded(4, q.C, F32)
        rm = Guarded(1, q.C, pdt, fill=f["rm_old"].to(pdt)) if q.running else None
        rv = Guarded(1, q.C, pdt, fill=f["rv_old"].to(pdt)) if q.running else None
        with Switches(lib, q.fuse):
            rc = lib.vgpu_bn_act_fwd_partials(_ptr(part), q.G, _ptr(x), y.ptr, _ptr(g), _ptr(b), rm and rm.ptr,
                                              rv and rv.ptr, coef.ptr, q.M, q.C, 0.0, mom, B.ACT[q.act], int(q.bf16),
                                              _stream())
            torch.cuda.synchronize()
        assert rc == 0, rc
        assert y.intact() and coef.intact() and (not q.running or (rm.intact() and rv.intact()))
        got[mom] = (y, coef, rm, rv)
        what = f"G {q.G}, {'fused' if q.fused else 'finalize + apply'}, momentum {mom}:"
        ref = torch.stack([f["s"], f["t"], f["mean"], f["invstd"]]).float()
        _same(coef.t, ref, f"{what} coef [s, t, mean, invstd][channel]")
        _same(y.t, round_to(B.act_ref(f["z"], q.act), BF), f"{what} y [row, channel]")
        if not q.running:
            break
        if mom == 0.25:
            _same(rm.t[0], round_to(0.75 * f["rm_old"] + 0.25 * f["mean"], F32).to(pdt), f"{what} running mean")
        else:
            _same(rm.t[0], round_to(f["mean"], pdt), f"{what} running mean")
            if q.bf16:
                _bf16_of(rv.t[0], f["unbiased"].float(), f"{what} running var")
            else:
                _ulp1(rv.t[0], f["unbiased"], f"{what} running var")


@pytest.mark.parametrize("q", B.PARTIALS, ids=lambda q: q.id)
def test_bn_backward_from_partials_exact(lib, q):
    """vgpu_bn_bwd_partials on synthetic integer pairs: d-gamma and d-beta EQUAL
    their sums; dx = s dz + cc x + b (+ add) within bf16's half-ulp; with and
    without add, and with null d-gamma / d-beta."""
    pb = B.bwd_partials_case(q.M, q.C)
    c = pb["case"]
    pdt = BF if q.bf16 else F32
    part = pb["partial"].float().cuda().contiguous()
    xd, dzd, addd = _dev(c.x, BF), _dev(c.dy, BF), _dev(c.add, BF)
    g, b = _dev(c.gamma, pdt), _dev(c.beta, pdt)
    mean, invstd = _dev(c.mean, F32), _dev(c.invstd, F32)
    s = c.gamma * c.invstd
    for with_add, null_grads in ((False, False), (True, False), (True, True)):
        dx, ws = Guarded(q.M, q.C), Guarded(4, q.C, F32)
        dg = None if null_grads else Guarded(1, q.C, pdt)
        db = None if null_grads else Guarded(1, q.C, pdt)
        with Switches(lib, q.fuse):
            rc = lib.vgpu_bn_bwd_partials(_ptr(part), q.G, _ptr(dzd), _ptr(xd), dx.ptr, _ptr(g), _ptr(b), _ptr(mean),
                                          _ptr(invstd), dg and dg.ptr, db and db.ptr, ws.ptr, q.M, q.C, int(q.bf16),
                                          _ptr(addd) if with_add else None, _stream())
            torch.cuda.synchronize()
        assert rc == 0, rc
        assert dx.intact() and ws.intact() and (null_grads or (dg.intact() and db.intact()))
        what = f"G {q.G}, {'fused' if q.fused else 'finalize + apply'}, add {with_add}:"
        if not null_grads:
            _same(db.t[0], round_to(pb["dbeta"], pdt), f"{what} dbeta")
            _same(dg.t[0], round_to(pb["dgamma"], pdt), f"{what} dgamma")
        rdx, bound = B.dx_ref(c.x.double(), c.dy.double(), c.add if with_add else None, s, c.mean, c.invstd,
                              pb["dgamma"], pb["dbeta"], q.M)
        _within(dx.t, rdx, bound, f"{what} dx [row, channel]")


# ---- Part C: statistics from the convolution's epilogue -------------------------------
class ConvMode:
    """vgpu_conv_set_tile_m / vgpu_conv_set_halo for one run, restored on exit."""
    SET = {"tile64": (64, 0), "tile128": (128, 0), "halo128": (0, 3), "halo256": (0, 2)}

    def __init__(self, lib, mode):
        self.lib, self.mode = lib, mode

    def __enter__(self):
        self.lib.vgpu_conv_set_tile_m(self.SET[self.mode][0])
        self.lib.vgpu_conv_set_halo(self.SET[self.mode][1])
        self.before = self.lib.vgpu_conv_halo_launches()

    def __exit__(self, *exc):
        self.lib.vgpu_conv_set_tile_m(0)
        self.lib.vgpu_conv_set_halo(-1)

    def check(self):
        assert self.lib.vgpu_conv_halo_launches() - self.before == int(self.mode.startswith("halo")), self.mode


CONV_PARAMS = [pytest.param(k, m, id=f"{k}-{m}") for k in B.CONV_KINDS for m in B.conv_modes(k)]


def _conv_bn(lib, case, kind, mode, bnx=None, coef=None, act=0):
    n, c, h, w, cout, ks, s, p, _ = B.CONV_KINDS[kind]
    M, G = case["M"], case["G"]
    x, wt, res = _dev(case["x"], BF), _dev(case["w"], BF), _dev(case["res"], BF)
    y, st = Guarded(M, cout), Guarded(G, 2 * cout, F32)
    run = ConvMode(lib, mode)
    with run:
        rc = lib.vgpu_conv2d_nhwc_bn(_ptr(x), _ptr(wt), y.ptr, _ptr(res), n, h, w, c, cout, ks, s, p, st.ptr, _ptr(bnx),
                                     _ptr(coef), act, 1, _stream())
        torch.cuda.synchronize()
        assert rc == 0, rc
        run.check()
    assert y.intact() and st.intact()
    return y.t, st.t.view(G, cout, 2)


@pytest.mark.parametrize("kind,mode", CONV_PARAMS)
def test_conv_epilogue_forward_statistics_exact(lib, kind, mode):
    """vgpu_conv2d_nhwc_bn, forward: the stored y is an exact integer and
    st[g, c] = (sum y, sum y**2) over each 64-row group EQUALS the int64 sums,
    on 64- and 128-row tiles and both halo tiles, with M % 64 != 0, images that
    straddle groups, 1x1, 3x3 stride 1 and 2, and a residual."""
    case = B.conv_case(kind)
    y, st = _conv_bn(lib, case, kind, mode)
    ry, rst = B.conv_fwd_ref(case)
    _same(y, round_to(ry, BF), f"{kind} {mode} y [row, channel]")
    _same(st, rst.float(), f"{kind} {mode} statistics [group, channel, (sum, sum of squares)]")


@pytest.mark.parametrize("act", list(B.ACT))
@pytest.mark.parametrize("kind,mode", [p for p in CONV_PARAMS if B.CONV_KINDS[p.values[0]][6] == 1])
def test_conv_epilogue_backward_statistics_exact(lib, kind, mode, act):
    """vgpu_conv2d_nhwc_bn with bnx: the conv's output (+ residual) is the
    gradient of a BatchNorm output whose input bnx has rows planted at z == 0 and
    z == 6; the stored dy * act'(z) and the pairs (sum, sum * x-hat) EQUAL the
    reference (integer mean, power-of-two s and invstd)."""
    case = B.conv_case(kind)
    v, rst, coef = B.conv_bwd_ref(case, act)
    y, st = _conv_bn(lib, case, kind, mode, _dev(case["bn"].x, BF), _dev(coef, F32), B.ACT[act])
    _same(y, round_to(v, BF), f"{kind} {mode} {act} stored dy * mask [row, channel]")
    _same(st, rst.float(), f"{kind} {mode} {act} statistics [group, channel, (sum, sum * x-hat)]")
