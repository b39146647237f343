"""Kernel selection of the convolution host path, without a GPU.

tests/golden/conv_plan_parent.json is a kernel trace of scripts/conv_plan_trace.py's
table, taken with VGPU_CONV_CUS = 8 and 256 on the commit before selection moved
into native/kernels/conv_plan.h: per row the return code, vgpu_conv2d_workspace's
answer and every (kernel, grid, workgroup) launched.  Here conv_plan.h, compiled
with g++, must name the same launches for every row.  The only normalisation is
the PRO template argument that conv_gemm_kernel had then (always true in a launch).

What this covers is conv_plan.h.  The argument checks that the entry points of
conv_gemm.hip make themselves (null operands of vgpu_conv2d_nhwc_bn, the masked and
pool entry points, the conv23 family) are mirrored here in Python so that every row
can be replayed; for those -1 rows the test compares Python with the golden file and
is no regression coverage of the .hip.  The GPU trace of scripts/conv_plan_trace.py
against the golden file is what checks them.
"""
from __future__ import annotations

import ctypes
import json
import re
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
GOLDEN = json.loads((REPO / "tests" / "golden" / "conv_plan_parent.json").read_text())
FAMILIES = ["unsupported", "gemm", "pro", "glds", "big", "halo"]
PLAN_FIELDS = "family nb KS BM BN CSM ST threads RES POST splits kper nM nN nmajor past_split".split()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    so = tmp_path_factory.mktemp("conv_plan") / "libconv_plan.so"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-shared", "-fPIC",
                    str(REPO / "native" / "tests" / "conv_plan_capi.cpp"), "-o", str(so)], check=True)
    lib = ctypes.CDLL(str(so))
    lib.conv_workspace_c.restype = ctypes.c_int64
    return lib


def _arr(vals):
    return (ctypes.c_int64 * len(vals))(*[int(v) for v in vals])


def _knobs(cus: int, s: dict):
    k = {"tile_m": 0, "big": -1, "halo": -1, "splitk": -1, **s["knobs"]}
    # no VGPU_CONV_BIG / VGPU_CONV_HALO / VGPU_CONV_1X1_BIG in the traced processes
    return _arr([cus, k["tile_m"], k["big"], k["halo"], k["splitk"], 2, 1, 0])


def _b(v) -> str:
    return "true" if v else "false"


def _launch(name: str, grid_x: int, grid_y: int, threads: int) -> list:
    return [name, [grid_x * threads, grid_y, 1], [threads, 1, 1]]


def _out_hw(s: dict, ks: int, pad: int) -> tuple[int, int]:
    # C++ division truncates towards zero
    return int((s["H"] + 2 * pad - ks) / s["stride"]) + 1, int((s["W"] + 2 * pad - ks) / s["stride"]) + 1


def _plan(lib, shape, knobs, last: int) -> dict:
    out = (ctypes.c_int64 * len(PLAN_FIELDS))()
    lib.conv_plan_c(shape, knobs, last, out)
    return dict(zip(PLAN_FIELDS, out))


def _conv2d(lib, cus: int, s: dict):
    """(rc, launches) of a vgpu_conv2d_* row: the entry point's own argument checks, then the plan."""
    ep, null = s["ep"], s["null"]
    ks, pad, stride = s["KS"], s["pad"], s["stride"]
    stats = res_stride = masked = 0
    post = ep == "post"
    res = s["res"] and "res" not in null
    knobs = _knobs(cus, s)
    if ep in ("conv", "plain"):
        if ("pscale" in null) != ("pshift" in null):
            return -1, []
    elif post:
        if {"qs", "qt", "res"} & set(null):
            return -1, []
        ks, pad, res = 1, 0, True
    elif ep == "bn":
        bnx, res_stride = bool(s.get("bnx")), s.get("res_stride", 1)
        if "stats" in null or (bnx and "bncoef" in null) or not 0 <= s.get("bnact", 0) <= 2:
            return -1, []
        if res_stride != 1 and (res_stride != 2 or not bnx or not res):
            return -1, []
        stats = 2 if bnx else 1
    else:  # masked, pool
        cout, stride, masked = s["Cout"], 1, 1
        oh, ow = s["H"] + 2 * pad - ks + 1, s["W"] + 2 * pad - ks + 1
        if ep == "pool":
            pk = s["pk"]
            if {"pidx", "gfull"} & set(null) or not 1 <= pk <= 15:
                return -1, []
            if oh < 1 or ow < 1 or s["N"] * oh * pk * ow * pk * cout * 2 >= 1 << 31:
                return -1, []
        if {"gmask", "gpart"} & set(null) or s["ws"] == "none" or cout % 8 or 256 % (cout // 8) or ks < 1 or pad < 0:
            return -1, []
        if oh < 1 or ow < 1:
            return -1, []
        shape0 = _arr([s["N"], s["H"], s["W"], s["C"], cout, ks, 1, pad, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0])
        if lib.conv_workspace_c(shape0, knobs) <= 0 or s.get("gpart_short"):
            return -1, []
    need = lib.conv_workspace_c(_arr([s["N"], s["H"], s["W"], s["C"], s["Cout"], s["KS"], s["stride"], s["pad"], 0, 0,
                                      s["pro"], 0, 0, 1, 0, 0, 0, 0]), knobs)
    ws_bytes = {"none": 0, "exact": need, "short": need - 4}[s["ws"]]
    shape = _arr([s["N"], s["H"], s["W"], s["C"], s["Cout"], ks, stride, pad, s["act"], bool(s["bias"]),
                  s["pro"] and ep in ("conv", "plain"), res, stats, res_stride or 1, post, masked, s["ws"] != "none",
                  ws_bytes])
    full, last = _plan(lib, shape, knobs, 0), _plan(lib, shape, knobs, 1)
    if "unsupported" in (FAMILIES[full["family"]], FAMILIES[last["family"]]):
        return -1, []
    launches = []
    oh, ow = _out_hw({**s, "stride": stride}, ks, pad)
    for n0 in range(0, s["N"], full["nb"]):
        p = last if s["N"] - n0 < full["nb"] else full
        fam = FAMILIES[p["family"]]
        m = p["nb"] * oh * ow
        assert p["nM"] == -(-m // p["BM"]) and p["nN"] == s["Cout"] // p["BN"]
        split = p["splits"] > 1
        name = {
            "gemm": "conv_gemm_kernel<{KS}, {BM}, {BN}, {r}>",
            "pro": "conv_pro_kernel<{KS}, {BM}, {BN}, {r}>",
            "glds": "conv_glds_kernel<{KS}, {BM}, {BN}, {r}, {CSM}, {ST}, {sp}, {po}>",
            "big": "conv_big_kernel<{r}, 4>",
            "halo": "conv_halo_kernel<{BM}, {BN}, {hp}, {ST}>",
        }[fam].format(**p, r=_b(p["RES"]), sp=_b(split), po=_b(p["POST"] and not split), hp=p["BM"] * 3 // 2)
        launches.append(_launch(name, p["nM"] * p["nN"], p["splits"], p["threads"]))
        # N-major halo placement: exactly when the filter is larger than 2.5 MiB (no trace shows it)
        assert p["nmajor"] == (fam == "halo" and s["Cout"] * ks * ks * s["C"] * 2 > 5 << 19)
        if split:
            assert p["splits"] * m * s["Cout"] * 4 <= ws_bytes
            assert (p["splits"] - 1) * p["kper"] < ks * ks * s["C"] // 64 <= p["splits"] * p["kper"]
            launches.append(_launch(f"splitk_reduce_kernel<{_b(p['POST'])}>", -(-m * (s["Cout"] // 8) // 256), 1, 256))
    return 0, launches


def _conv23(lib, s: dict):
    ep, null, c, stride = s["ep"], set(s["null"]), s["C"], s["stride"]
    nxt, post, sc = ep in ("c231", "c231sc"), ep == "c23post", ep == "c231sc"
    if post and {"qs", "qt"} & null:
        return -1, []
    if nxt and "w1n" in null:
        return -1, []
    if sc and ({"xpre", "wsc"} & null or c != 64 or s["Csc"] != 64 or stride != 1):
        return -1, []
    bm = lib.conv23_bm_c(c, nxt, post, sc)
    if not bm or stride < 1 or s["N"] < 1 or "b2" in null or (not sc and "res" in null):
        return -1, []
    if nxt and {"b1n", "psn", "ptn", "h1n"} & null:
        return -1, []
    oh, ow = _out_hw(s, 3, 1)
    if oh < 1 or ow < 1:
        return -1, []
    if (2 ** 31 - 1) // max(s["H"] * s["W"] * c * 2, oh * ow * 4 * c * 2) < 1:
        return -1, []
    m = s["N"] * oh * ow  # every traced conv23 row is one slice
    name = f"conv23_kernel<{bm}, {c}, {_b(nxt)}, 3, 256, {_b(post)}, {_b(sc)}>"
    return 0, [_launch(name, (m + bm - 1) // bm, 1, 256)]


def _normalised(launches: list) -> list:
    drop_pro = re.compile(r"^(conv_gemm_kernel<\d+, \d+, \d+), true, ")
    return [[drop_pro.sub(r"\1, ", name), grid, wg] for name, grid, wg in launches]


@pytest.mark.parametrize("cus", sorted(GOLDEN, key=int))
def test_plan_reproduces_parent_trace(lib, cus):
    rows = GOLDEN[cus]
    assert len(rows) > 150
    bad = []
    for i, row in enumerate(rows):
        s = row["spec"]
        if s["ep"].startswith("c23"):
            rc, launches = _conv23(lib, s)
        else:
            rc, launches = _conv2d(lib, int(cus), s)
            knobs = _knobs(int(cus), s)
            ws = lib.conv_workspace_c(_arr([s["N"], s["H"], s["W"], s["C"], s["Cout"], s["KS"], s["stride"], s["pad"],
                                            0, 0, s["pro"], 0, 0, 1, 0, 0, 0, 0]), knobs)
            if ws != row["ws"]:
                bad.append((i, "workspace", ws, row["ws"]))
        if rc != row["rc"] or launches != _normalised(row["launches"]):
            bad.append((i, s, rc, launches, row["rc"], row["launches"]))
    assert not bad, bad[:5]


def test_golden_covers_every_family_and_unsupported():
    names = {l[0].split("<")[0] for rows in GOLDEN.values() for r in rows for l in r["launches"]}
    assert names == {"conv_gemm_kernel", "conv_pro_kernel", "conv_glds_kernel", "conv_big_kernel", "conv_halo_kernel",
                     "splitk_reduce_kernel", "conv23_kernel"}
    for rows in GOLDEN.values():
        assert sum(r["rc"] == -1 for r in rows) >= 60 and all(r["rc"] in (0, -1) for r in rows)
        assert all(r["launches"] == [] for r in rows if r["rc"] == -1)


def test_last_slice_plans_its_own_tile(lib):
    """A batch that runs in slices plans each slice: the short last one may take the other tile."""
    # 1x1 prologue conv 64 -> 128 on 128x128 images: the output is 4 MiB per image, 511 images per slice;
    # N = 512 leaves a last slice of one image, whose 128 tiles of 128 rows are below 1.5 per CU
    shape = _arr([512, 128, 128, 64, 128, 1, 1, 0, 0, 0, 1, 0, 0, 1, 0, 0, 0, 0])
    knobs = _arr([256, 0, -1, -1, -1, 2, 1, 0])
    full, last = _plan(lib, shape, knobs, 0), _plan(lib, shape, knobs, 1)
    assert full["nb"] == (2 ** 31 - 1) // (128 * 128 * 128 * 2) == 511 and last["nb"] == 1
    assert FAMILIES[full["family"]] == FAMILIES[last["family"]] == "gemm"
    assert [(p["BM"], p["nM"], p["nN"]) for p in (full, last)] == [(128, 511 * 128, 1), (64, 256, 1)]


def test_env_big_counts_as_forced_only_once_taken_over(lib):
    """VGPU_CONV_BIG=1 picks the 256x256 tile from the start, but turns split-K off only once
    conv_gemm.hip has taken it over into the setter's global (forced_big 1), as it always did."""
    shape = _arr([1, 8, 8, 512, 256, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 1, 1 << 30])
    env, taken = _arr([256, 0, -1, -1, -1, 1, 1, 0]), _arr([256, 0, 1, -1, -1, 1, 1, 0])
    assert _plan(lib, shape, env, 0)["splits"] == 2 and not _plan(lib, shape, env, 0)["past_split"]
    p = _plan(lib, shape, taken, 0)
    assert (FAMILIES[p["family"]], p["splits"], p["past_split"]) == ("big", 1, 1)
    unsplit = _arr([1, 8, 8, 512, 256, 1, 1, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0])
    p = _plan(lib, unsplit, env, 0)
    assert (FAMILIES[p["family"]], p["past_split"]) == ("big", 1)
