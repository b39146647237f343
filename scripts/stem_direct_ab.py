#!/usr/bin/env python3
"""In-process A/B of the fused stem's two changes -- bands and direct input --
against another build of the kernels library (the parent commit's, built beside
this tree), on the ResNet-50 flagship shape (b=50, 346²) with the post epilogue
as the runner calls it.  Four variants, each captured in a graph of REPS calls
and replayed in interleaved rounds; outputs compared bit for bit.

    parent        other library: space-to-depth kernel + vgpu_stem_pool_post_nhwc
    banded_x      this library:  space-to-depth kernel + vgpu_stem_pool_post_nhwc (bands)
    direct_band1  this library:  vgpu_stem_pool_x_nhwc, one pooled row per band
    direct        this library:  vgpu_stem_pool_x_nhwc, bands by the rule

    python scripts/stem_direct_ab.py build_ab/parent/vgpu/_lib/libvgpu_kernels.so [out.jsonl] [batch] [rounds]

Prints one JSON line per round (us per call of each variant) and a summary line.
"""
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vgpu.native import load_kernels  # noqa: E402
from vgpu.ops import conv as C  # noqa: E402

other = ctypes.CDLL(os.path.abspath(sys.argv[1]))
OUT = sys.argv[2] if len(sys.argv) > 2 else None
B = int(sys.argv[3]) if len(sys.argv) > 3 else 50
ROUNDS = int(sys.argv[4]) if len(sys.argv) > 4 else 12
REPS = 20
vp, ci = ctypes.c_void_p, ctypes.c_int
other.vgpu_stem_pool_post_nhwc.argtypes = [vp] * 5 + [ci] * 3 + [vp]
other.vgpu_stem_pool_post_nhwc.restype = ci
other.vgpu_stem_space_to_depth.argtypes = [vp, vp] + [ci] * 6 + [vp]
other.vgpu_stem_space_to_depth.restype = ci
cur = load_kernels()

torch.manual_seed(0)
x = torch.randn(B, 3, 346, 346, device="cuda").to(torch.bfloat16).contiguous(memory_format=torch.channels_last)
w = C.stem_weight_s2d((torch.randn(64, 3, 7, 7, device="cuda") * 0.1).to(torch.bfloat16))
qs = torch.rand(64, device="cuda") + 0.5
qt = torch.rand(64, device="cuda") - 0.5
n, _, h, wd = x.shape
_, _, hs, ws = C.stem_s2d_shape(h, wd)
X = torch.empty((n, 16, hs, ws), dtype=x.dtype, device="cuda", memory_format=torch.channels_last)
ref = C.conv2d(C.maxpool3s2(C.stem_conv(x, w)),
               torch.eye(64).reshape(64, 64, 1, 1).to(torch.bfloat16).cuda().contiguous(
                   memory_format=torch.channels_last), pro=(qs, qt))
VARIANTS = ("parent", "banded_x", "direct_band1", "direct")
outs = {k: torch.zeros_like(ref) for k in VARIANTS}


def run(k, s):
    y = outs[k]
    if k in ("parent", "banded_x"):
        lib = other if k == "parent" else cur
        rc = lib.vgpu_stem_space_to_depth(vp(x.data_ptr()), vp(X.data_ptr()), n, h, wd, 3, hs, ws, s)
        assert rc == 0, (k, rc)
        rc = lib.vgpu_stem_pool_post_nhwc(vp(X.data_ptr()), vp(w.data_ptr()), vp(y.data_ptr()), vp(qs.data_ptr()),
                                          vp(qt.data_ptr()), n, hs, ws, s)
    else:
        rc = cur.vgpu_stem_pool_x_nhwc(vp(x.data_ptr()), vp(w.data_ptr()), vp(y.data_ptr()), vp(qs.data_ptr()),
                                       vp(qt.data_ptr()), n, h, wd, s)
    assert rc == 0, (k, rc)


graphs = {}
side = torch.cuda.Stream()
for k in VARIANTS:
    cur.vgpu_stem_set_band(1 if k == "direct_band1" else 0)  # read at launch, so fixed in the captured graph
    with torch.cuda.stream(side):
        run(k, vp(side.cuda_stream))  # warm: code object load
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(REPS):
            run(k, vp(torch.cuda.current_stream().cuda_stream))
    graphs[k] = g
cur.vgpu_stem_set_band(0)
for k in VARIANTS:
    graphs[k].replay()
torch.cuda.synchronize()
same = {k: bool(torch.equal(outs[k], ref)) for k in VARIANTS}

lines = []
for r in range(ROUNDS):
    order = VARIANTS[r % 4:] + VARIANTS[:r % 4]
    row = {"round": r}
    for k in order:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        graphs[k].replay()
        e1.record()
        torch.cuda.synchronize()
        row[k] = round(e0.elapsed_time(e1) * 1000 / REPS, 1)  # us per call
    lines.append(row)
    print(json.dumps(row), flush=True)
summary = {"batch": B, "reps_per_graph": REPS, "bit_identical": same}
for k in VARIANTS:
    v = sorted(row[k] for row in lines)
    summary[k] = {"median": v[len(v) // 2], "min": v[0], "max": v[-1]}
print(json.dumps(summary))
if OUT:
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as f:
        for row in lines + [summary]:
            f.write(json.dumps(row) + "\n")
assert all(same.values()), same
