"""tests/_conv_exact.py without a GPU: both conditions of its docstring hold for the
reference of every case, the reference generator agrees with vgpu.ops.conv.conv2d_ref,
conv_plan.h (g++, native/tests/conv_plan_capi.cpp) names each case's kernel at any CU
count, and the table reaches every ST = 0 entry of conv_kernel() and every edge listed
in assert_coverage."""
from __future__ import annotations

import pytest
import torch

import _conv_exact as X
from test_conv_plan_cpu import FAMILIES, _arr, _plan, lib  # noqa: F401  (lib: the compiled conv_plan.h)

CUS = (8, 64, 256, 304)
IDS = [c.name for c in X.CASES]


def _shape_row(case: X.Case, ws_bytes: int):
    n, h, w, c, cout, ks, stride, pad = case.shape
    return _arr([n, h, w, c, cout, ks, stride, pad, case.act, case.bias != "none", case.pro, case.res, 0, 1,
                 case.post, 0, case.splits > 1, ws_bytes])


def _knob_row(case: X.Case, cus: int):
    # no VGPU_CONV_BIG / VGPU_CONV_HALO / VGPU_CONV_1X1_BIG in the environment
    return _arr([cus, case.tile_m, case.big, case.halo, case.splitk, 2, 1, 0])


def _kernel_of(p: dict) -> str:
    fam = FAMILIES[p["family"]]
    res = bool(p["RES"])
    if fam == "gemm":
        return X.k_gemm(p["KS"], p["BM"], p["BN"], res)
    if fam == "pro":
        return X.k_pro(p["KS"], p["BM"], p["BN"], res)
    if fam == "glds":
        split = p["splits"] > 1
        assert p["ST"] == 0
        return X.k_glds(p["KS"], p["BM"], p["BN"], res, csm=p["CSM"], split=split, post=bool(p["POST"]) and not split)
    if fam == "big":
        return X.k_big(res)
    if fam == "halo":
        assert p["BN"] == 128 and p["ST"] == 0
        return X.k_halo(p["BM"])
    return "unsupported"


def _planned(lib, case: X.Case, cus: int) -> dict:
    full = _plan(lib, _shape_row(case, case.workspace), _knob_row(case, cus), 0)
    last = _plan(lib, _shape_row(case, case.workspace), _knob_row(case, cus), 1)
    assert full == last and full["nb"] == case.shape[0], "the exact cases run as one batch slice"
    return full


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_conditions_hold_on_the_reference(case):
    o, r = X.operands(case), X.reference(case)
    assert X.representable(case, r), {k: int(r[k].abs().max()) for k in ("conv", "pre", "y", "out")}
    assert X.visible(case, o)
    n, h, w, c, cout, ks, stride, pad = case.shape
    assert r["want"].shape == (n, *case.out_hw, cout) and r["want"].dtype == torch.bfloat16
    assert all(t.numel() * 2 <= 72 << 20 for t in (o["x"], o["w"], r["want"])), "tensors stay under about 64 MB"
    if case.scheme != "dense":
        assert torch.equal(r["want"].to(torch.int64), r["out"].to(torch.int64))  # bf16 holds it exactly
        assert int(o["x"].abs().max()) == 1 and int(o["w"].abs().max()) == 1
        # one weight per reduction index in every 64-channel output block
        assert bool(((o["w"] != 0).view(cout // 64, 64, -1).sum(1) == 1).all())
    else:
        assert case.ktiles * 64 <= 576 and int(r["conv"].abs().max()) > X.BF16_EXACT  # the store does round
    if case.act:
        assert int(r["pre"].min()) < 0 < int(r["pre"].max())
        if case.act == 2:
            assert int(r["pre"].max()) > 6
    if case.pro:
        px, s, t = X.prologue_value(case, o), o["s"], o["t"]
        raw = o["x"] * s + t
        assert bool((raw < 0).any()) and bool((px != 0).flatten(0, 2).any(0).all()) and bool((t > 0).any())
        assert int(px.max()) <= (5 if case.scheme == "dense" else 3)
    if case.post:
        assert int(r["post_pre"].min()) < 0 < int(r["post_pre"].max())
        clamped = (r["out"] == 0).flatten(0, 2).all(0)
        assert set(o["qs"].tolist()) == {-1, 1, 2} and not bool(clamped.all())
        assert bool((r["out"] == 0).any())


@pytest.mark.parametrize("case", X.SMALL, ids=[c.name for c in X.SMALL])
def test_reference_agrees_with_conv2d_ref(case):
    """The library's own fp32 reference, fed the same integers, gives the same integers."""
    from vgpu.ops.conv import conv2d_ref
    o, r = X.operands(case), X.reference(case)
    n, h, w, c, cout, ks, stride, pad = case.shape
    bf = torch.bfloat16
    y = conv2d_ref(o["x"].permute(0, 3, 1, 2).to(bf), o["w"].permute(0, 3, 1, 2).to(bf),
                   None if o["bias"] is None else o["bias"].float(), stride=stride, padding=pad, act=X.ACTS[case.act],
                   pro=(o["s"].float(), o["t"].float()) if case.pro else None,
                   residual=None if o["res"] is None else o["res"].permute(0, 3, 1, 2).float())
    assert y.dtype == torch.float32 and int(r["conv"].abs().max()) < X.FP32_EXACT
    assert torch.equal(y.permute(0, 2, 3, 1).to(torch.int64), r["y"])


def test_small_set_spans_the_families():
    assert {c.family for c in X.SMALL} == {"gemm", "pro", "glds", "split", "post", "big", "halo"}
    assert any(c.pro for c in X.SMALL) and any(c.shape[5] == 4 for c in X.SMALL)


@pytest.mark.parametrize("case", X.CASES, ids=IDS)
def test_plan_names_the_kernel_at_any_cu_count(lib, case):
    n, h, w, c, cout, ks, stride, pad = case.shape
    assert case.tile_m in (0, 64, 128) and case.big in (0, 1) and case.halo in (0, 2, 3)
    assert case.splitk == 0 or case.splitk > 1
    if case.family in ("gemm", "pro", "glds"):
        assert case.tile_m in (64, 128)
    plans = [_planned(lib, case, cus) for cus in CUS]
    assert all(p == plans[0] for p in plans), plans
    p = plans[0]
    assert FAMILIES[p["family"]] == case.plan_family
    assert _kernel_of(p) == case.kernel
    assert (p["BM"], p["BN"], p["splits"]) == (case.bm, case.bn, case.splits)
    assert p["nM"] == -(-case.M // case.bm) and p["nN"] == cout // case.bn
    for cus in CUS:
        assert lib.conv_workspace_c(_shape_row(case, 0), _knob_row(case, cus)) == case.workspace
    if case.splits > 1:
        assert (p["splits"] - 1) * p["kper"] < case.ktiles <= p["splits"] * p["kper"]
        # a byte short and the conv is refused rather than run unsplit
        short = _plan(lib, _shape_row(case, case.workspace - 4), _knob_row(case, 256), 0)
        assert FAMILIES[short["family"]] == "unsupported"


def test_table_reaches_every_planned_kernel(lib):
    rows = [(c, _planned(lib, c, 256)) for c in X.CASES]
    reached = {_kernel_of(p) for _, p in rows} | {c.reduce for c in X.CASES if c.reduce}
    want = X.all_planned_kernels()
    assert len(want) == 64
    assert reached == want, (sorted(want - reached), sorted(reached - want))
    X.assert_coverage(rows)


def test_kernel_list_matches_the_source():
    """conv_kernel()'s tables hold what all_planned_kernels() spells out: 62 with ST = 0."""
    import re
    from pathlib import Path
    src = (Path(__file__).resolve().parents[1] / "native" / "kernels" / "conv_gemm.hip").read_text()
    body = src[src.index("ConvKernel conv_kernel("):src.index("#undef VGPU_BN_RES")]
    tiles = len(re.findall(r"VGPU_TILES\((\w+)\)", body))              # ST = 0 tables of 16: gemm, pro, glds
    stats = len(re.findall(r"VGPU_TILES\(conv_glds_kernel, 0, [12]\)", body))
    listed = re.findall(r"(conv_(?:glds|big|halo)_kernel<[^>]*>)", body)
    st0 = [k for k in listed if not re.fullmatch(r"conv_halo_kernel<\d+, \d+, \d+, [12]>", k)]
    assert (tiles, stats, len(st0)) == (3, 2, 14) and tiles * 16 + len(st0) == 62


@pytest.mark.parametrize("tile_m", (64, 128))
def test_narrow_conv_with_a_residual_is_refused(lib, tile_m):
    """conv_kernel() has no residual form of the narrow kernels (its table is [BM] alone): the plan
    must refuse the request, where it used to name the residual-free kernel and drop the operand."""
    case = next(c for c in X.CASES if c.name == "glds-narrow-bm64")
    shape = list(_shape_row(case, 0))
    for cus in CUS:
        knobs = _arr([cus, tile_m, 0, 0, 0, 2, 1, 0])
        assert FAMILIES[_plan(lib, _arr(shape), knobs, 0)["family"]] == "glds"
        with_res = shape[:11] + [1] + shape[12:]
        assert all(FAMILIES[_plan(lib, _arr(with_res), knobs, last)["family"]] == "unsupported" for last in (0, 1))
