#!/usr/bin/env python3
"""attn_prefill alone against F.scaled_dot_product_attention(is_causal=True)
on the same random values: H = 32, KVH = 8, hd = 128, B = 1, start = 0.

SDPA takes K and V with as many heads as Q, so it is timed twice: with the
repeat_interleave that grouped-query attention needs in front of it, and
without (K / V repeated once, outside the window).  Each window is `iters`
calls between two device events after `warm` untimed calls; the three paths
alternate within a round, and the median, minimum and maximum over the rounds
are printed.  FLOP/s count the causal half only: 4 · hd · S(S+1)/2 per head.
Outputs are compared before anything is timed.

    python scripts/prefill_attn_bench.py [--sizes 512,2048,8192] [--rounds 5] [--out FILE]
"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

H, KVH, HD = 32, 8, 128


def window(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters  # ms per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="512,2048,8192")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured without one")
    from vgpu.ops import prefill as P
    rows = []
    for S in (int(s) for s in a.sizes.split(",")):
        g = torch.Generator(device="cuda").manual_seed(S)
        q = torch.randn(1, S, H, HD, generator=g, device="cuda").bfloat16()
        k = torch.randn(1, KVH, S, HD, generator=g, device="cuda").bfloat16()
        v = torch.randn(1, KVH, S, HD, generator=g, device="cuda").bfloat16()
        out = torch.empty(1, S, H * HD, dtype=torch.bfloat16, device="cuda")
        qt = q.transpose(1, 2)  # [1, H, S, hd], the view Attention.forward hands to SDPA
        kr, vr = k.repeat_interleave(H // KVH, dim=1), v.repeat_interleave(H // KVH, dim=1)
        scale = HD ** -0.5
        paths = {
            "native": lambda: P.attn_prefill(q, k, v, 0, out, scale),
            "sdpa_with_repeat": lambda: F.scaled_dot_product_attention(
                qt, k.repeat_interleave(H // KVH, dim=1), v.repeat_interleave(H // KVH, dim=1), is_causal=True),
            "sdpa_alone": lambda: F.scaled_dot_product_attention(qt, kr, vr, is_causal=True),
        }
        paths["native"]()
        ref = paths["sdpa_alone"]().transpose(1, 2).reshape(1, S, H * HD)
        diff = (out.float() - ref.float()).abs().max().item()
        flops = 4.0 * HD * (S * (S + 1) / 2) * H
        iters = max(10, min(200, int(2e12 / flops)))  # a window of tens of milliseconds or more
        for fn in paths.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        ms = {name: [] for name in paths}
        for _ in range(a.rounds):
            for name, fn in paths.items():
                ms[name].append(window(fn, iters))
        row = {"S": S, "iters": iters, "max_abs_diff_vs_sdpa": round(diff, 5)}
        for name, t in ms.items():
            med = statistics.median(t)
            row[name] = {"ms_median": round(med, 4), "ms_min": round(min(t), 4), "ms_max": round(max(t), 4),
                         "tflops_median": round(flops / med / 1e9, 1)}
        rows.append(row)
        print("PREFILL_ATTN " + json.dumps(row), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"H": H, "KVH": KVH, "hd": HD, "B": 1, "start": 0, "rows": rows}, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
