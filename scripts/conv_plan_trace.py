#!/usr/bin/env python3
"""Which kernels the convolution host path launches, row by row.

Runs a fixed table of convs (ROWS) once each through the exported entry points
of native/kernels/conv_gemm.hip and prints, per row, one JSON line: the row's
index and spec, the return code and vgpu_conv2d_workspace's answer.  Before
each row a marker kernel (vgpu_fill_pattern) runs with row + 1 workgroups, so
a kernel trace of the process splits into rows by itself:

    VGPU_CONV_CUS=8 rocprofv3 --kernel-trace --output-format csv -d DIR -o run -- \\
        python3 scripts/conv_plan_trace.py > DIR/rows.jsonl
    python3 scripts/conv_plan_trace.py --golden 8=DIR [256=DIR2 ...] > tests/golden/conv_plan_parent.json

VGPU_CONV_CUS is cached per process: one process per value.  With 8 CUs every
grid-fill threshold of the selection is crossed by shapes of a few thousand
output pixels.  tests/test_conv_plan_cpu.py replays the golden file against
native/kernels/conv_plan.h without a GPU.

Rows that expect -1 for an oversized tensor ("dummy": true) pass 4 KiB
buffers: the contract is that -1 comes before any launch.
"""
from __future__ import annotations

import csv
import ctypes
import glob
import json
import os
import re
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

DEFAULTS = dict(ep="conv", N=1, H=8, W=8, C=64, Cout=64, KS=1, stride=1, pad=0, act=0, pro=False, res=False,
                bias=None, ws="none", knobs={}, null=[], dummy=False)
KNOB_RESET = dict(tile_m=0, big=-1, halo=-1, splitk=-1)


def r(**kw) -> dict:
    bad = set(kw) - set(DEFAULTS) - {"bnx", "bnact", "res_stride", "pk", "Csc", "gpart_short"}
    assert not bad, bad
    return kw


def _rows() -> list[dict]:
    big = dict(H=40, W=40)  # M = 1600: 13 tiles of 128 rows, past the 12 that 8 CUs ask for
    k3 = dict(KS=3, pad=1)
    rows = [
        # -- prologue convs on conv_pro_kernel ...
        r(pro=True, C=256, Cout=128, **big),
        r(pro=True, C=256, Cout=128, res=True),
        r(pro=True, C=192, Cout=128),
        r(pro=True, C=2048, Cout=128),
        r(pro=True, **k3, Cout=192),
        r(pro=True, **k3, Cout=128, res=True, **big),
        r(pro=True, **k3, Cout=128, act=1, bias="f32"),
        # ... and the four reasons they take conv_gemm_kernel: K <= 2 steps, Cout == 64, C > 2048, padded 1x1
        r(pro=True, C=64, Cout=128),
        r(pro=True, C=128, Cout=128, res=True),
        r(pro=True, C=64, Cout=128, res=True, **big),
        r(pro=True, C=128, Cout=192),
        r(pro=True, **k3, Cout=64, res=True),
        r(pro=True, **k3, Cout=64, **big),
        r(pro=True, C=256, Cout=64),
        r(pro=True, C=2112, Cout=128),
        r(pro=True, C=256, Cout=128, pad=1),
        r(pro=True, C=256, Cout=128, pad=1, res=True, **big),
        # -- LDS-DMA convs: KS, residual, rows128_ok (C 192 / 256, Cout 64 / 128), the narrow stem form
        r(),
        r(ep="plain", Cout=128, act=2, bias="f32"),
        r(C=256, Cout=128, **big),
        r(C=192, Cout=128, **big),
        r(C=256, Cout=64, **big),
        r(C=256, Cout=128, res=True, **big),
        r(C=256, Cout=128, act=1, bias="bf16"),
        r(**k3, Cout=128, stride=2, H=80, W=80),
        r(**k3, Cout=128, res=True, **big),
        r(**k3, Cout=64, res=True),
        r(**k3, Cout=64),
        r(KS=3, pad=0, Cout=128),
        r(C=16, KS=4, H=11, W=11),
        r(C=16, KS=4, H=43, W=43),
        r(C=16, KS=4, Cout=128, H=43, W=43),
        r(C=16, KS=4, H=11, W=11, ws="exact"),
        # -- 256x256 tile: tiles below / at the CU count, forced on at C = 128, forced off
        r(C=1024, Cout=256, H=32, W=56),
        r(C=1024, Cout=256, H=32, W=64),
        r(C=1024, Cout=256, H=32, W=64, res=True),
        r(C=1024, Cout=256, H=32, W=64, stride=2),
        r(C=512, Cout=256, H=32, W=64),
        r(C=128, Cout=256, knobs=dict(big=1)),
        r(C=128, Cout=256, res=True, knobs=dict(big=1)),
        r(C=64, Cout=256, knobs=dict(big=1)),
        r(C=1024, Cout=256, H=32, W=64, knobs=dict(big=0)),
        # -- halo: BM 256 / 128, W = 16 fits, W = 32 / 48 fall back, Cout = 64 falls back, forced modes
        r(**k3, Cout=128, H=80, W=16),
        r(**k3, Cout=128, H=64, W=16),
        r(**k3, Cout=128, H=48, W=48),
        r(**k3, Cout=128, H=8, W=32),
        r(**k3, Cout=128, H=64, W=32),
        r(**k3, Cout=64, H=80, W=16),
        r(**k3, C=512, Cout=512, H=8, W=16),
        r(**k3, Cout=128, H=80, W=16, knobs=dict(halo=0)),
        r(**k3, Cout=128, H=8, W=16, knobs=dict(halo=1)),
        r(**k3, Cout=128, H=8, W=16, knobs=dict(halo=2)),
        r(**k3, Cout=128, H=48, W=48, knobs=dict(halo=2)),
        r(**k3, Cout=128, H=80, W=16, knobs=dict(halo=3)),
        r(**k3, Cout=128, H=64, W=32, knobs=dict(halo=3)),
        # -- forced tile rows
        r(C=256, Cout=128, knobs=dict(tile_m=128)),
        r(pro=True, C=256, Cout=128, **big, knobs=dict(tile_m=64)),
        # -- statistics, forward and backward, on glds and halo; res_stride 2
        r(ep="bn", Cout=128),
        r(ep="bn", **k3, stride=2),
        r(ep="bn", C=256, Cout=128, **big),
        r(ep="bn", C=1024, Cout=256, H=32, W=64),
        r(ep="bn", **k3, Cout=128, H=80, W=16),
        r(ep="bn", **k3, Cout=128, H=8, W=16),
        r(ep="bn", **k3, Cout=128, H=48, W=48),
        r(ep="bn", Cout=128, res=True, bnx=True, bnact=1),
        r(ep="bn", Cout=64, bnx=True, bnact=2),
        r(ep="bn", **k3, Cout=128, H=8, W=16, bnx=True, bnact=1),
        r(ep="bn", **k3, Cout=128, H=9, W=9, res=True, bnx=True, bnact=1, res_stride=2),
        r(ep="bn", **k3, Cout=64, res=True, bnx=True, bnact=0, res_stride=2, **big),
        r(ep="bn", null=["stats"]),
        r(ep="bn", bnx=True, null=["bncoef"]),
        r(ep="bn", bnact=3),
        r(ep="bn", bnact=-1),
        r(ep="bn", res=True, res_stride=2),
        r(ep="bn", bnx=True, res_stride=2),
        r(ep="bn", res=True, bnx=True, res_stride=3),
        r(ep="bn", C=16, KS=4, H=11, W=11),
        r(ep="bn", C=96),
        r(ep="bn", N=4, H=2048, W=2048, dummy=True),
        r(ep="bn", N=4, H=4096, W=4096, res=True, bnx=True, res_stride=2, dummy=True),
        # -- split-K: with / without a workspace, split counts, forced 0 / 3, post reduce, masked, masked-pool
        r(**k3, C=128, Cout=128, ws="exact"),
        r(**k3, C=128, Cout=128),
        r(**k3, C=512, Cout=128, ws="exact"),
        r(**k3, C=512, Cout=128, W=16, ws="exact"),
        r(**k3, C=512, Cout=128, W=24, ws="exact"),
        r(**k3, C=512, Cout=128, W=32, ws="exact"),
        r(**k3, C=512, Cout=128, ws="exact", **big),
        r(C=512, Cout=64, ws="exact", res=True, act=1, bias="f32"),
        r(C=512, Cout=192, ws="exact"),
        r(C=256, Cout=128, ws="exact"),
        r(C=192, Cout=128, ws="exact"),
        r(**k3, C=512, Cout=128, ws="exact", stride=2, H=16, W=16),
        r(**k3, C=512, Cout=128, ws="exact", knobs=dict(splitk=0)),
        r(**k3, C=512, Cout=128, ws="exact", knobs=dict(splitk=3)),
        r(**k3, C=512, Cout=128, ws="exact", knobs=dict(splitk=3), **big),
        r(**k3, C=64, Cout=128, ws="exact", knobs=dict(splitk=3)),
        r(**k3, C=512, Cout=128, ws="short"),
        r(**k3, C=512, Cout=128, ws="exact", pro=True),
        r(**k3, C=512, Cout=128, ws="exact", knobs=dict(halo=1)),
        r(**k3, C=512, Cout=128, ws="exact", knobs=dict(tile_m=64)),
        r(**k3, C=512, Cout=128, ws="exact", knobs=dict(tile_m=128)),
        r(C=512, Cout=256, ws="exact", knobs=dict(big=1)),
        r(C=512, Cout=256, ws="exact", knobs=dict(big=0)),
        r(**k3, C=512, Cout=128, ws="exact", knobs=dict(halo=1, splitk=3)),
        r(ep="post", C=512, Cout=128, ws="exact"),
        r(ep="post", C=512, Cout=64, ws="exact"),
        r(ep="post", C=512, Cout=128, ws="short"),
        r(ep="masked", **k3, C=128, Cout=128, ws="exact"),
        r(ep="masked", C=512, Cout=64, ws="exact"),
        r(ep="pool", **k3, C=128, Cout=128, ws="exact", pk=2),
        r(ep="pool", **k3, C=128, Cout=64, ws="exact", pk=3),
        # the masked entry points' -1s
        r(ep="masked", **k3, C=128, Cout=128, ws="exact", null=["gmask"]),
        r(ep="masked", **k3, C=128, Cout=128, ws="exact", null=["gpart"]),
        r(ep="masked", **k3, C=128, Cout=128, ws="none"),
        r(ep="masked", **k3, C=128, Cout=192, ws="exact"),
        r(ep="masked", KS=3, pad=-1, C=128, Cout=128, ws="exact"),
        r(ep="masked", KS=3, pad=0, H=2, W=2, C=128, Cout=128, ws="exact"),
        r(ep="masked", **k3, C=128, Cout=128, ws="exact", **big),
        r(ep="masked", **k3, C=128, Cout=128, ws="exact", knobs=dict(splitk=0)),
        r(ep="masked", **k3, C=128, Cout=128, ws="exact", gpart_short=True),
        r(ep="masked", **k3, C=128, Cout=128, ws="short"),
        r(ep="masked", **k3, N=4, H=2048, W=2048, ws="exact", knobs=dict(splitk=3), dummy=True),
        r(ep="pool", **k3, C=128, Cout=128, ws="exact", pk=2, null=["pidx"]),
        r(ep="pool", **k3, C=128, Cout=128, ws="exact", pk=2, null=["gfull"]),
        r(ep="pool", **k3, C=128, Cout=128, ws="exact", pk=0),
        r(ep="pool", **k3, C=128, Cout=128, ws="exact", pk=16),
        r(ep="pool", **k3, C=128, Cout=128, ws="exact", pk=2, null=["gmask"]),
        r(ep="pool", **k3, C=128, Cout=128, ws="exact", pk=2, **big),
        r(ep="pool", **k3, C=128, Cout=128, ws="exact", pk=2, gpart_short=True),
        r(ep="pool", **k3, C=128, Cout=128, N=64, H=256, W=256, pk=2, ws="exact", knobs=dict(splitk=3), dummy=True),
        # -- post: BM 64 / 128 x BN 64 / 128; a 256x256-eligible shape returns -1 with nothing launched
        r(ep="post"),
        r(ep="post", Cout=128),
        r(ep="post", knobs=dict(tile_m=128)),
        r(ep="post", Cout=128, knobs=dict(tile_m=128)),
        r(ep="post", Cout=128, stride=2, **big),
        r(ep="post", C=1024, Cout=256, H=32, W=64),
        r(ep="post", C=1024, Cout=256, H=32, W=56),
        r(ep="post", C=128, Cout=256, knobs=dict(big=1)),
        r(ep="post", null=["qs"]),
        r(ep="post", null=["qt"]),
        r(ep="post", null=["res"]),
        r(ep="post", N=4, H=2048, W=2048, dummy=True),
        # -- each -1 of the plain conv
        r(act=3),
        r(C=96),
        r(C=16, KS=4, H=11, W=11, pro=True),
        r(C=16, KS=4, H=11, W=11, stride=2),
        r(KS=5, H=11, W=11),
        r(Cout=96),
        r(stride=0),
        r(pad=-1),
        r(N=0),
        r(pro=True, null=["pshift"]),
        r(pro=True, null=["pscale"]),
        r(KS=3, H=2, W=2),
        r(H=4096, W=4096, dummy=True),
        # -- the seven conv23 variants and their -1s
        r(ep="c23", N=2, C=64),
        r(ep="c23", N=2, C=64, stride=2, H=9, W=9),
        r(ep="c23post", N=2, C=64),
        r(ep="c231", N=2, C=64),
        r(ep="c231sc", N=2, C=64, Csc=64),
        r(ep="c23", N=2, C=128),
        r(ep="c23post", N=2, C=128, stride=2),
        r(ep="c231", N=2, C=128, H=5, W=7),
        r(ep="c23", C=192),
        r(ep="c23", C=64, stride=0),
        r(ep="c23", C=64, N=0),
        r(ep="c23", C=64, H=0),
        r(ep="c23", C=64, null=["b2"]),
        r(ep="c23", C=64, null=["res"]),
        r(ep="c23post", C=64, null=["qs"]),
        r(ep="c23post", C=64, null=["qt"]),
        r(ep="c231", C=64, null=["w1n"]),
        r(ep="c231", C=64, null=["b1n"]),
        r(ep="c231", C=64, null=["psn"]),
        r(ep="c231", C=64, null=["h1n"]),
        r(ep="c231sc", C=128, Csc=64),
        r(ep="c231sc", C=64, Csc=128),
        r(ep="c231sc", C=64, Csc=64, stride=2),
        r(ep="c231sc", C=64, Csc=64, null=["xpre"]),
        r(ep="c231sc", C=64, Csc=64, null=["wsc"]),
        r(ep="c23", C=64, H=32768, W=32768, dummy=True),
    ]
    return [{**DEFAULTS, **row} for row in rows]


ROWS = _rows()


def out_hw(s: dict) -> tuple[int, int]:
    ks, pad = (3, 1) if s["ep"].startswith("c23") else (s["KS"], s["pad"])
    return (s["H"] + 2 * pad - ks) // s["stride"] + 1 if s["stride"] > 0 else 0, \
        (s["W"] + 2 * pad - ks) // s["stride"] + 1 if s["stride"] > 0 else 0


def run_rows() -> int:
    import torch
    from vgpu.native import load_kernels

    lib = load_kernels()
    dev = torch.device("cuda:0")
    vp, ci, i64 = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64
    stream = vp(torch.cuda.current_stream().cuda_stream)
    marker = torch.zeros((len(ROWS) + 1) * 4096, dtype=torch.uint8, device=dev)
    dummy = torch.zeros(4096, dtype=torch.uint8, device=dev)
    keep = []

    def buf(nbytes: int, s: dict, name: str):
        if name in s["null"]:
            return None
        if s["dummy"]:
            return vp(dummy.data_ptr())
        t = torch.zeros(max(int(nbytes), 16), dtype=torch.uint8, device=dev)
        keep.append(t)
        return vp(t.data_ptr())

    setters = dict(tile_m=lib.vgpu_conv_set_tile_m, big=lib.vgpu_conv_set_big, halo=lib.vgpu_conv_set_halo,
                   splitk=lib.vgpu_conv_set_splitk)
    for i, s in enumerate(ROWS):
        keep.clear()
        for k, v in {**KNOB_RESET, **s["knobs"]}.items():
            setters[k](ci(v))
        N, H, W, C, Cout, KS, st, pad = (s[k] for k in ("N", "H", "W", "C", "Cout", "KS", "stride", "pad"))
        OH, OW = out_hw(s)
        M = max(N * OH * OW, 0)
        ep = s["ep"]
        need = None
        if ep.startswith("c23"):
            c4 = 4 * C
            x = buf(N * H * W * C * 2, s, "x")
            w2, b2, w3 = buf(C * 9 * C * 2, s, "w2"), buf(C * 4, s, "b2"), buf(c4 * C * 2, s, "w3")
            res, y = buf(M * c4 * 2, s, "res"), buf(M * c4 * 2, s, "y")
            shape = (ci(N), ci(H), ci(W), ci(C))
            if ep == "c23":
                rc = lib.vgpu_conv23_nhwc(x, w2, b2, w3, res, y, *shape, ci(st), stream)
            elif ep == "c23post":
                rc = lib.vgpu_conv23_post_nhwc(x, w2, b2, w3, res, y, buf(c4 * 4, s, "qs"), buf(c4 * 4, s, "qt"),
                                               *shape, ci(st), stream)
            else:
                nxt = (buf(C * c4 * 2, s, "w1n"), buf(C * 4, s, "b1n"), buf(c4 * 4, s, "psn"), buf(c4 * 4, s, "ptn"),
                       buf(M * C * 2, s, "h1n"))
                if ep == "c231":
                    rc = lib.vgpu_conv231_nhwc(x, w2, b2, w3, res, y, *nxt, *shape, ci(st), stream)
                else:
                    rc = lib.vgpu_conv231_sc_nhwc(x, w2, b2, w3, buf(N * H * W * 64 * 2, s, "xpre"),
                                                  buf(c4 * 64 * 2, s, "wsc"), y, *nxt, *shape, ci(s["Csc"]), ci(st),
                                                  stream)
        else:
            need = int(lib.vgpu_conv2d_workspace(N, H, W, C, Cout, KS, st, pad, int(s["pro"])))
            x, w = buf(N * H * W * C * 2, s, "x"), buf(Cout * KS * KS * C * 2, s, "w")
            y = buf(M * Cout * 2, s, "y")
            rs = s.get("res_stride", 1)
            res = buf(N * ((OH + 1) // 2) * ((OW + 1) // 2) * Cout * 2 if rs == 2 else M * Cout * 2, s, "res") \
                if s["res"] or ep == "post" else None
            bias = buf(Cout * 4, s, "bias") if s["bias"] else None
            act = s["act"] | (256 if s["bias"] == "bf16" else 0)
            ps = buf(C * 4, s, "pscale") if s["pro"] else None
            pt = buf(C * 4, s, "pshift") if s["pro"] else None
            wsb = {"none": 0, "exact": need, "short": need - 4}[s["ws"]]
            ws = buf(wsb, s, "ws") if s["ws"] != "none" else None
            dims = (ci(N), ci(H), ci(W), ci(C), ci(Cout))
            if ep == "plain":
                rc = lib.vgpu_conv2d_nhwc(x, w, y, res, bias, ps, pt, *dims, ci(KS), ci(st), ci(pad), ci(act), stream)
            elif ep == "conv":
                rc = lib.vgpu_conv2d_nhwc_ws(x, w, y, res, bias, ps, pt, *dims, ci(KS), ci(st), ci(pad), ci(act), ws,
                                             i64(wsb), stream)
            elif ep == "post":
                rc = lib.vgpu_conv2d_post_nhwc_ws(x, w, y, res, buf(Cout * 4, s, "qs"), buf(Cout * 4, s, "qt"), *dims,
                                                  ci(st), ws, i64(wsb), stream)
            elif ep == "bn":
                stats = buf(((M + 63) // 64) * Cout * 8, s, "stats")
                bnx = buf(M * Cout * 2, s, "bnx") if s.get("bnx") else None
                coef = buf(4 * Cout * 4, s, "bncoef") if s.get("bnx") else None
                rc = lib.vgpu_conv2d_nhwc_bn(x, w, y, res, *dims, ci(KS), ci(st), ci(pad), stats, bnx, coef,
                                             ci(s.get("bnact", 0)), ci(rs), stream)
            else:
                blocks = (M * (Cout // 8) + 255) // 256
                gpb = blocks * Cout * 4 - (4 if s.get("gpart_short") else 0)
                gpart, nblk = buf(gpb, s, "gpart"), ctypes.c_int(0)
                if ep == "masked":
                    rc = lib.vgpu_conv2d_masked_splitk(x, w, y, *dims, ci(KS), ci(pad), buf(M * Cout * 2, s, "gmask"),
                                                       gpart, i64(gpb), ws, i64(wsb), ctypes.byref(nblk), stream)
                else:
                    pk = s["pk"]
                    full = M * max(pk, 1) ** 2 * Cout * 2
                    rc = lib.vgpu_conv2d_masked_pool_splitk(x, w, *dims, ci(KS), ci(pad), buf(M * Cout, s, "pidx"),
                                                            ci(pk), buf(full, s, "gmask"), buf(full, s, "gfull"),
                                                            gpart, i64(gpb), ws, i64(wsb), ctypes.byref(nblk), stream)
        torch.cuda.synchronize()
        lib.vgpu_fill_pattern(vp(marker.data_ptr()), ctypes.c_uint64((i + 1) * 4096), ctypes.c_uint32(i), stream)
        torch.cuda.synchronize()
        print(json.dumps({"row": i, "spec": s, "rc": int(rc), "ws": need, "marker": i + 1}), flush=True)
    for k, v in KNOB_RESET.items():
        setters[k](ci(v))
    return 0


def _launches(d: str) -> list[list]:
    """The trace's dispatches in start order as [name, grid xyz, workgroup xyz], markers included."""
    recs = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        recs += list(csv.DictReader(open(f)))
    recs.sort(key=lambda t: int(t["Start_Timestamp"]))
    out = []
    for t in recs:
        name = re.sub(r"\(anonymous namespace\)::", "", t["Kernel_Name"])
        name = re.sub(r"^void ", "", name).split("(")[0]
        out.append([name, [int(t[f"Grid_Size_{a}"]) for a in "XYZ"], [int(t[f"Workgroup_Size_{a}"]) for a in "XYZ"]])
    return out


def golden(pairs: list[str]) -> int:
    """rows.jsonl + kernel trace of each run -> the golden document on stdout."""
    doc = {}
    for pair in pairs:
        cus, d = pair.split("=", 1)
        rows = [json.loads(ln) for ln in open(os.path.join(d, "rows.jsonl")) if ln.startswith("{")]
        per_row, pending = {}, []
        for name, grid, wg in _launches(d):
            if name.endswith("fill_kernel"):  # the marker that closes a row: grid = its "marker" value
                per_row[grid[0] // wg[0]] = pending
                pending = []
            elif re.match(r"(conv_|conv23_|splitk_reduce)", name):
                pending.append([name, grid, wg])
        assert not pending, "conv kernels after the last marker"
        assert len(rows) == len(ROWS) == len(per_row), (len(rows), len(ROWS), len(per_row))
        doc[cus] = [{"spec": row["spec"], "rc": row["rc"], "ws": row["ws"],
                     "launches": per_row.get(row["marker"], [])} for row in rows]
    body = []  # one compact object per row: a new row is a one-line diff
    for cus, rows in doc.items():
        body.append(json.dumps(cus) + ": [\n" + ",\n".join(json.dumps(r, separators=(",", ":")) for r in rows) + "\n]")
    print("{\n" + ",\n".join(body) + "\n}")
    return 0


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--golden":
        sys.exit(golden(sys.argv[2:]))
    sys.exit(run_rows())
