#!/usr/bin/env python3
"""In-process A/B of the decode GEMV on Llama-3-8B's four projection shapes at
B = 1, 2, 4, 8: vgpu_skinny_fwd over bf16 weights against vgpu_gemv_fp8 over
e4m3 codes.  Each variant is a hipGraph of calls that walk a pool of distinct
weights of at least --pool-mb, so that every call streams from HBM as a
decode step does and not from the 256 MB MALL; variants alternate within each
round, the median over rounds is reported.  One JSON line per (shape, B)."""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vgpu.ops import decode as D, fp8 as F  # noqa: E402

SHAPES = {"wqkv": (6144, 4096), "wo": (4096, 4096), "w13": (28672, 4096), "w2": (4096, 14336)}


def graph_of(calls):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for c in calls:
            c()
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for c in calls:
            c()
    return g


def replay_us(g, calls):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pool-mb", type=int, default=1024)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--batches", default="1,2,4,8")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    F._lib()
    D._lib()
    torch.manual_seed(0)
    lines = []
    for name, (N, K) in SHAPES.items():
        copies = max(8, -(-a.pool_mb * (1 << 20) // (N * K)))  # the fp8 pool; the bf16 pool is twice its bytes
        w16 = [(torch.randn(N, K, device="cuda") * 0.02).to(torch.bfloat16) for _ in range(copies)]
        w8 = [F.quantize(w) for w in w16]
        for B in [int(b) for b in a.batches.split(",")]:
            x = torch.randn(B, K, device="cuda").to(torch.bfloat16)
            y = torch.empty(B, N, dtype=torch.bfloat16, device="cuda")
            variants = {"bf16": [lambda w=w: D.gemv(x, w, y) for w in w16],
                        "fp8": [lambda c=c, s=s: F.gemv_fp8(x, c, s, y) for c, s in w8]}
            graphs = {k: graph_of(v) for k, v in variants.items()}
            times = {k: [] for k in graphs}
            for _ in range(a.rounds):
                for k, g in graphs.items():
                    times[k].append(replay_us(g, copies))
            res = {"layer": name, "N": N, "K": K, "B": B, "copies": copies}
            for k, t in times.items():
                us = statistics.median(t)
                wbytes = N * K * (2 if k == "bf16" else 1)
                res[k] = {"us": round(us, 2), "min": round(min(t), 2), "max": round(max(t), 2),
                          "weight_TBps": round(wbytes / us / 1e6, 2)}
            res["fp8_over_bf16_time"] = round(res["fp8"]["us"] / res["bf16"]["us"], 3)
            print(json.dumps(res), flush=True)
            lines.append(res)
        del w16, w8
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            for r in lines:
                f.write(json.dumps(r) + "\n")


if __name__ == "__main__":
    main()
