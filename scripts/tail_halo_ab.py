#!/usr/bin/env python3
"""In-process A/B of the fused tails' halo form of phase 1 (conv23_kernel<..., HALO>)
against the ring form, on the six stride-1 tail calls of the ResNet-V2-50 flagship
(b=50, 346²: stage 1 at 87 x 87 with C = 64, stage 2 at 44 x 44 with C = 128) with
the operand forms the runner uses:

    b0  conv231 with the projection shortcut in the tail   C = 64
    b1  conv231 (identity residual)                        C = 64
    b2  conv23 with the post epilogue                      C = 64
    b4  conv231                                            C = 128
    b5  conv231                                            C = 128
    b6  conv23 with the post epilogue                      C = 128

Variants, each captured in a graph of REPS calls and replayed in interleaved rounds
whose order rotates; outputs compared bit for bit:

    ring     this library, vgpu_conv23_set_halo(0)
    halo     this library, vgpu_conv23_set_halo(1)
    NAME     (optional, --lib NAME=LIB, repeatable) another build of the kernels library,
             e.g. the parent commit's; a NAME that starts with "halo" runs with that
             library's own vgpu_conv23_set_halo(1) (a build with another ring depth)
    timing   (optional, --timing-only LIB) a library whose results are wrong on purpose
             (an experiment's timing ceiling); never compared

    python scripts/tail_halo_ab.py [--lib parent=build_ab/parent/vgpu/_lib/libvgpu_kernels.so]
                                   [--timing-only LIB] [--out out.jsonl] [--batch 50] [--rounds 12]

Prints one JSON line per round (us per call of each tail and variant) and a summary line.
"""
import argparse
import ctypes
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vgpu.native import load_kernels  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lib", action="append", default=[], metavar="NAME=LIB")
ap.add_argument("--timing-only", default=None)
ap.add_argument("--out", default=None)
ap.add_argument("--batch", type=int, default=50)
ap.add_argument("--rounds", type=int, default=12)
args = ap.parse_args()
REPS = 20
vp, ci = ctypes.c_void_p, ctypes.c_int
CL = torch.channels_last


def declare(lib):
    lib.vgpu_conv23_post_nhwc.argtypes = [vp] * 8 + [ci] * 5 + [vp]
    lib.vgpu_conv231_nhwc.argtypes = [vp] * 11 + [ci] * 5 + [vp]
    lib.vgpu_conv231_sc_nhwc.argtypes = [vp] * 12 + [ci] * 6 + [vp]
    for f in (lib.vgpu_conv23_post_nhwc, lib.vgpu_conv231_nhwc, lib.vgpu_conv231_sc_nhwc):
        f.restype = ci
    return lib


cur = declare(load_kernels())
libs = {"ring": cur, "halo": cur}
for spec in args.lib:
    name, path = spec.split("=", 1)
    libs[name] = declare(ctypes.CDLL(os.path.abspath(path)))
    if name.startswith("halo"):
        libs[name].vgpu_conv23_set_halo.argtypes = [ci]
        libs[name].vgpu_conv23_set_halo(1)
if args.timing_only:
    libs["timing"] = declare(ctypes.CDLL(os.path.abspath(args.timing_only)))
VARIANTS = tuple(libs)
COMPARED = tuple(v for v in VARIANTS if v != "timing")
TAILS = (("b0", "sc", 64, 87), ("b1", "next", 64, 87), ("b2", "post", 64, 87),
         ("b4", "next", 128, 44), ("b5", "next", 128, 44), ("b6", "post", 128, 44))

gen = torch.Generator(device="cpu").manual_seed(0)


def bf(shape, scale=1.0, relu=False):
    t = torch.randn(shape, generator=gen) * scale
    if relu:
        t = t.clamp_min(0)
    return t.to(torch.bfloat16).cuda().contiguous(memory_format=CL)


def fl(n, lo, hi):
    return (torch.rand((n,), generator=gen) * (hi - lo) + lo).cuda().contiguous()


def operands(c, hw):
    n = args.batch
    return dict(
        n=n, c=c, hw=hw,
        h=bf((n, c, hw, hw), relu=True), w2=bf((c, c, 3, 3), (2.0 / (9 * c)) ** 0.5), b2=fl(c, -0.5, 0.5),
        w3=bf((4 * c, c, 1, 1), (2.0 / c) ** 0.5), res=bf((n, 4 * c, hw, hw)),
        xp=bf((n, 64, hw, hw), relu=True), wsc=bf((4 * c, 64, 1, 1), (2.0 / 64) ** 0.5),
        w1n=bf((c, 4 * c, 1, 1), (2.0 / (4 * c)) ** 0.5), b1n=fl(c, -0.5, 0.5),
        ps=fl(4 * c, 0.5, 1.5), pt=fl(4 * c, -0.5, 0.5))


ops = {(c, hw): operands(c, hw) for c, hw in {(t[2], t[3]) for t in TAILS}}
outs = {}
for name, form, c, hw in TAILS:
    for v in VARIANTS:
        n = args.batch
        outs[name, v] = tuple(torch.empty((n, k, hw, hw), dtype=torch.bfloat16, device="cuda",
                                          memory_format=CL).zero_() for k in (4 * c, c))


def p(t):
    return vp(t.data_ptr())


def run(name, form, c, hw, v, s):
    lib, o = libs[v], ops[c, hw]
    y, h1 = outs[name, v]
    n = o["n"]
    if form == "sc":
        rc = lib.vgpu_conv231_sc_nhwc(p(o["h"]), p(o["w2"]), p(o["b2"]), p(o["w3"]), p(o["xp"]), p(o["wsc"]), p(y),
                                      p(o["w1n"]), p(o["b1n"]), p(o["ps"]), p(o["pt"]), p(h1), n, hw, hw, c, 64, 1, s)
    elif form == "next":
        rc = lib.vgpu_conv231_nhwc(p(o["h"]), p(o["w2"]), p(o["b2"]), p(o["w3"]), p(o["res"]), p(y), p(o["w1n"]),
                                   p(o["b1n"]), p(o["ps"]), p(o["pt"]), p(h1), n, hw, hw, c, 1, s)
    else:
        rc = lib.vgpu_conv23_post_nhwc(p(o["h"]), p(o["w2"]), p(o["b2"]), p(o["w3"]), p(o["res"]), p(y), p(o["ps"]),
                                       p(o["pt"]), n, hw, hw, c, 1, s)
    assert rc == 0, (name, v, rc)


graphs, halo_taken = {}, {}
side = torch.cuda.Stream()
for name, form, c, hw in TAILS:
    for v in VARIANTS:
        cur.vgpu_conv23_set_halo(1 if v == "halo" else 0)  # read at launch, so fixed in the captured graph
        before = cur.vgpu_conv23_halo_launches()
        with torch.cuda.stream(side):
            run(name, form, c, hw, v, vp(side.cuda_stream))  # warm: code object load
        torch.cuda.synchronize()
        took = cur.vgpu_conv23_halo_launches() - before
        assert took == 0 or v == "halo", (name, v)
        if v == "halo":
            halo_taken[name] = bool(took)  # False: the plan rule keeps the ring for this shape
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=side):
            for _ in range(REPS):
                run(name, form, c, hw, v, vp(torch.cuda.current_stream().cuda_stream))
        graphs[name, v] = g
cur.vgpu_conv23_set_halo(-1)
for g in graphs.values():
    g.replay()
torch.cuda.synchronize()
same = {name: all(torch.equal(a, b) for v in COMPARED for a, b in zip(outs[name, v], outs[name, "ring"]))
        for name, *_ in TAILS}

lines = []
for r in range(args.rounds):
    k = r % len(VARIANTS)
    order = VARIANTS[k:] + VARIANTS[:k]
    row = {"round": r}
    for name, *_ in TAILS:
        for v in order:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            graphs[name, v].replay()
            e1.record()
            torch.cuda.synchronize()
            row[f"{name}.{v}"] = round(e0.elapsed_time(e1) * 1000 / REPS, 1)  # us per call
    lines.append(row)
    print(json.dumps(row), flush=True)
summary = {"batch": args.batch, "reps_per_graph": REPS, "bit_identical": same, "halo_taken": halo_taken}
for name, *_ in TAILS:
    for v in VARIANTS:
        vals = sorted(row[f"{name}.{v}"] for row in lines[1:])  # round 0 runs on a cold clock
        summary[f"{name}.{v}"] = {"median": vals[len(vals) // 2], "min": vals[0], "max": vals[-1]}
print(json.dumps(summary))
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for row in lines + [summary]:
            f.write(json.dumps(row) + "\n")
assert all(same.values()), same
