"""The inputs of tests/test_gpu_bn_exact.py, checked without a GPU: x is exact
in bf16, every partial sum stays an integer below 2**24, a single lost or
doubled row moves the saved statistics by >= 16 fp32 ulp (the GPU test allows
1), the fp64 reference equals torch's batch_norm in fp64, the backward sums
and the synthetic partials are exact, and the case lists reach every plan and
branch of bn_nhwc.hip that tests/_bn_exact.py mirrors."""
import pytest
import torch
import torch.nn.functional as F

import _bn_exact as B
from _exact import FP32_EXACT, I64

F64 = torch.float64
BF = torch.bfloat16


def test_case_lists_cover_every_plan_and_branch():
    B.assert_bn_coverage()


def test_plan_mirror_on_known_shapes():
    """Figures that can be read off bn_nhwc.hip by hand."""
    assert B.plain_kind(768, 64) == 2 and B.plain_kind(769, 64) == 1 and B.plain_kind(768, 96) == 0
    assert B.plain_kind(100, 64, fuse=False) == 0
    p = B.make_plan(10753, 96)     # 21 rows a pass, 4 passes a block: 84 rows, G = 129 just past M = 10752
    assert (p["rpb"], p["dead"], p["rows_per_block"], p["G"]) == (21, 4, 84, 129)
    assert B.make_plan(10752, 96)["G"] == 128
    p = B.make_plan(1000, 520)
    assert (p["chunk"], p["nchunks"], p["last_chunk"], p["rpb"]) == (512, 2, 8, 4)
    assert B.make_plan(3001, 96, True, (2, 8))["rows_per_block"] == 21 * 72
    assert B.fused_grid(769, 64) == (1, 7, 110) and B.fused_grid(64, 64) == (1, 1, 64)
    assert B.fused_grid(4097, 1024) == (16, 16, 257)
    assert B.fused_ok(160, 64) and not B.fused_ok(161, 64) and not B.fused_ok(2, 96) and not B.fused_ok(2, 64, False)
    assert B.workspace(1000, 96) == 2 * 12 * 96 + 4 * 96


def test_ulps_and_bf16_choices():
    one = torch.tensor([1.0, -1.0, 0.0, 3.5])
    up = torch.nextafter(one, torch.full_like(one, 9.0))
    assert B.ulps(one, up).tolist() == [1, 1, 1, 1] and B.ulps(one, one).tolist() == [0, 0, 0, 0]
    assert int(B.ulps(torch.tensor([float("nan")]), torch.tensor([1.0]))) > 1 << 30
    tie = torch.tensor([1.00390625, 1.5])            # 1 + 2**-8: a bf16 tie; 1.5: exact
    ch = B.bf16_choices(tie)
    assert len(set(ch[:, 0].tolist())) == 2 and len(set(ch[:, 1].tolist())) == 1


def _fwd_inputs(p):
    """(name, x) for a case: the dense input and, for single-row cases, one per edge row."""
    yield "dense", B.fwd_input(p.M, p.C, "dense") if p.M > 1 else B.fwd_input(1, p.C, "dense")
    if p.single:
        for r in B.edge_rows(p.M, p.C, p.fuse != 0, p.tuning):
            yield f"row {r}", B.fwd_input(p.M, p.C, "single", r)


@pytest.mark.parametrize("p", B.PLAIN, ids=lambda p: p.id)
def test_forward_inputs_are_exact_and_sensitive(p):
    cc = B.const_channel(p.C)
    live = torch.ones(p.C, dtype=torch.bool)
    live[cc] = False
    for name, x in _fwd_inputs(p):
        assert x.shape == (p.M, p.C) and int(x.abs().max()) <= 256
        assert torch.equal(x.to(BF).to(I64), x), name                       # exact in bf16
        e = x - x[0]
        assert int((e * e).sum(0).max()) < FP32_EXACT and int(e.abs().sum(0).max()) < FP32_EXACT
        assert len(set(x[0].tolist())) >= min(p.C, len(B.OFFSETS)) and int(x[0].abs().max()) >= 192
        st = B.fwd_stats(x)
        assert float(st.var[cc]) == 0.0 and abs(float(st.invstd[cc]) * B.EPS ** 0.5 - 1) < 1e-15  # the clamp's
        if p.M == 1:
            assert float(st.var.max()) == 0.0
            continue
        if name == "dense":
            assert bool((e[1:, live] != 0).all())                           # no row equal to row 0
            rows = slice(1, None)
        else:
            r = int(name.split()[1])
            assert bool((e[r, live] != 0).all()) and int((e != 0).any(1).sum()) == 1
            rows = slice(r, r + 1)
        moved = B.row_sensitivity(x, st)[rows][:, live]
        assert int(moved.min()) >= 16, (name, int(moved.min()))
        # the reference is torch's batch_norm in fp64
        gamma, beta, rm, rv = B.fwd_params(p.C)
        rm2, rv2 = rm.clone(), rv.clone()
        yt = F.batch_norm(x.double(), rm2, rv2, gamma, beta, True, 1.0, B.EPS)
        z, delta = B.fwd_ref(x, st, gamma, beta, "none")
        torch.testing.assert_close(z, yt, rtol=0, atol=1e-9)
        torch.testing.assert_close(rm2, st.mean, rtol=1e-14, atol=1e-13)
        torch.testing.assert_close(rv2, st.unbiased, rtol=1e-11, atol=1e-13)
        assert bool((delta >= 0).all()) and float(delta[:, live].max()) < 0.01   # the fp32 slack: a small absolute term
        # where the mean is not an integer the 0.25-momentum update is still close to dyadic: |old| is a multiple of 4
        assert torch.equal(rm, (rm / 4).round() * 4) and torch.equal(rm.to(BF).double(), rm)
    for t in B.fwd_params(p.C):
        assert torch.equal(t.to(BF).double(), t)                            # bf16 parameters are the same numbers


def test_y_bound_sees_one_bf16_step():
    """A y one bf16 step away from the correctly rounded one misses the bound
    on nearly every element (all those whose fp32 slack 2 * delta is below half
    a bf16 step minus the rounding already spent)."""
    p = B.PLAIN[10]
    x = B.fwd_input(p.M, p.C, "dense")
    gamma, beta, _, _ = B.fwd_params(p.C)
    z, delta = B.fwd_ref(x, B.fwd_stats(x), gamma, beta, "none")
    y = z.to(BF)
    assert bool(((y.double() - z).abs() <= B.y_bound(z, delta)).all())
    for to in (float("inf"), float("-inf")):
        off = torch.nextafter(y, torch.full_like(y, to))
        missed = ((off.double() - z).abs() > B.y_bound(z, delta)).double().mean().item()
        assert missed > 0.7, missed


def _bwd_cases(p):
    yield "dense", B.bwd_case(p.M, p.C, "dense", affine=p.affine)
    if p.single:
        for r in B.edge_rows(p.M, p.C, p.fuse != 0, p.tuning, backward=True)[::2]:
            yield f"row {r}", B.bwd_case(p.M, p.C, "single", r, affine=p.affine)


@pytest.mark.parametrize("p", [p for p in B.PLAIN if p.M > 1], ids=lambda p: p.id)
def test_backward_inputs_are_exact(p):
    for name, c in _bwd_cases(p):
        for t in (c.x, c.dy, c.add):
            assert torch.equal(t.to(BF).to(I64), t)
        assert int(c.dy.abs().max()) <= 4 and int((c.x - c.mean.to(I64)).abs().max()) <= 8
        assert torch.equal(c.mean, c.mean.round()) and set(c.invstd.tolist()) <= {1.0, 0.5, 0.25}
        gamma = torch.ones(p.C, dtype=F64) if c.gamma is None else c.gamma
        beta = torch.zeros(p.C, dtype=F64) if c.beta is None else c.beta
        s = gamma * c.invstd
        t = beta - c.mean * s
        assert bool((torch.log2(s.abs()) == torch.log2(s.abs()).round()).all()) and torch.equal(beta, beta.round())
        for v in (s, t, c.mean, c.invstd, gamma, beta):
            assert torch.equal(v.float().double(), v)
        assert torch.equal(gamma.to(BF).double(), gamma) and torch.equal(beta.to(BF).double(), beta)
        z = c.x.double() * s + t
        assert torch.equal(z.float().double(), z)          # the kernel's fma(x, s, t) is this number
        assert bool((z[c.z0] == 0).all()) and bool((z[c.z6] == 6).all())
        for act in B.ACT:
            dg, db, dx, bound, terms = B.bwd_ref(c, act, True)
            assert 4 * terms < FP32_EXACT and 4 * float(dg.abs().max()) < FP32_EXACT
            assert torch.equal(dg * 4, (dg * 4).round()) and torch.equal(db, db.round())
            assert float(db.abs().max()) > 0 and float(dg.abs().max()) > 0
            assert float((bound - 2.0 ** -8 * dx.abs()).max()) < 0.01  # the fp32 slack: a small absolute term
        if name == "dense":
            assert bool((c.dy != 0).all())
            if p.M >= 4:
                # the planted edges carry gradient: a mask of z >= 0 or z <= 6 would move both sums
                assert bool(c.z0.any()) and bool(c.z6.any())
                zero_hit = (c.dy * c.z0).abs().sum(0)
                six_hit = (c.dy * c.z6).abs().sum(0)
                assert int((zero_hit > 0).sum()) >= p.C // 2 and int((six_hit > 0).sum()) >= p.C // 4
        else:
            r = int(name.split()[1])
            assert int((c.dy != 0).any(1).sum()) == 1 and bool((c.dy[r] != 0).all())
            assert bool(((z[r] > 0) & (z[r] < 6)).all())   # the one row passes every mask
    # the sums through autograd (the saved statistics are chosen, not x's own, so they are constants here), and
    # dx in batch_norm backward's own arrangement
    if p.M * p.C <= 1 << 16 and p.affine:
        c = B.bwd_case(p.M, p.C, "dense")
        for act in B.ACT:
            g, b = c.gamma.clone().requires_grad_(), c.beta.clone().requires_grad_()
            xhat = (c.x.double() - c.mean) * c.invstd
            y = xhat * g + b
            y = F.relu(y) if act == "relu" else F.hardtanh(y, 0.0, 6.0) if act == "relu6" else y
            y.backward(c.dy.double())
            dg, db, dx, _, _ = B.bwd_ref(c, act, False)
            assert torch.equal(dg, g.grad) and torch.equal(db, b.grad)
            dz = c.dy.double() * B.act_mask((xhat * c.gamma + c.beta), act)
            want = (c.gamma * c.invstd) * (dz - dz.mean(0) - xhat * (dz * xhat).mean(0))
            torch.testing.assert_close(dx, want, rtol=1e-13, atol=1e-13)


@pytest.mark.parametrize("q", B.PARTIALS, ids=lambda q: q.id)
def test_partials_cases_are_exact(q):
    f = B.fwd_partials_case(q.M, q.C)
    G = f["G"]
    assert G == (q.M + 63) // 64 and f["partial"].shape == (G, q.C, 2)
    part = f["partial"]
    assert bool((part != 0).all()) and int(part.abs().max()) < FP32_EXACT
    assert torch.equal(part.float().to(I64), part)
    if G > 1:
        assert bool((part < 0).any())
    S1, S2 = part[..., 0].sum(0), part[..., 1].sum(0)
    assert int(part.abs().sum(0).max()) < 2 ** 53
    assert torch.equal(S1.double() / q.M, f["mean"]) and torch.equal(S2.double() / q.M - f["mean"] ** 2, f["var"])
    assert set(f["var"].tolist()) == {1.0, 4.0, 16.0} and torch.equal(1.0 / torch.sqrt(f["var"]), f["invstd"])
    for k in ("s", "t", "mean", "invstd", "z"):
        assert torch.equal(f[k].float().double(), f[k]), k
    for k in ("gamma", "beta", "rm_old", "rv_old"):
        assert torch.equal(f[k].to(BF).double(), f[k]), k
    assert torch.equal(f["z"], f["x"].double() * f["s"] + f["t"])
    assert torch.equal(f["z"].to(BF).double(), f["z"]) and torch.equal(f["x"].to(BF).to(I64), f["x"])
    if q.M >= 4:
        assert bool((f["z"] == 0).any()) and bool((f["z"] == 6).any()) and bool((f["z"] > 6).any())
    rm = 0.75 * f["rm_old"] + 0.25 * f["mean"]
    assert torch.equal(rm.float().double(), rm)
    b = B.bwd_partials_case(q.M, q.C)
    part = b["partial"]
    assert part.shape == (G, q.C, 2) and bool((part != 0).all()) and int(part.abs().sum(0).max()) < FP32_EXACT
    assert torch.equal(part[..., 0].sum(0).double(), b["dbeta"])
    assert torch.equal(part[..., 1].sum(0).double(), b["dgamma"])


@pytest.mark.parametrize("kind", list(B.CONV_KINDS))
def test_conv_statistics_cases_are_exact(kind):
    """The stored outputs are integers exact in bf16, every group sum is exact
    in fp32 in any order, M is no multiple of 64 and images straddle groups."""
    n, c, h, w, cout, ks, s, p, has_res = B.CONV_KINDS[kind]
    case = B.conv_case(kind)
    M, G = case["M"], case["G"]
    assert M % 64 != 0 and (case["oh"] * case["ow"]) % 64 != 0 and G >= 2 and (case["res"] is not None) == has_res
    assert bool(((case["w"].reshape(cout, -1) != 0).sum(0) == 1).all())
    y, st = B.conv_fwd_ref(case)
    assert 0 < int(y.abs().max()) <= 128 and st.shape == (G, cout, 2)
    assert int((y * y).sum(0).max()) < FP32_EXACT and torch.equal(st.float().double(), st)
    assert torch.equal(st[..., 0].sum(0), y.sum(0).double()) and torch.equal(st[..., 1].sum(0), (y * y).sum(0).double())
    assert bool((st[..., 1] > 0).all())                                   # every group of every channel is visible
    bn = case["bn"]
    assert torch.equal(bn.x.to(BF).to(I64), bn.x)
    for act in B.ACT:
        v, sb, coef = B.conv_bwd_ref(case, act)
        assert torch.equal(coef.float().double(), coef) and torch.equal(v.to(BF).double(), v)
        xhat = (bn.x.double() - bn.mean) * bn.invstd
        assert 4 * float((v * xhat).abs().sum(0).max()) < FP32_EXACT and torch.equal(sb.float().double(), sb)
        if act != "none":
            assert bool((v == 0).any()) and bool(((y != 0) & bn.z0).any())
        if act == "relu6":
            assert bool(((y != 0) & bn.z6).any())                         # a gradient sits on z == 6
