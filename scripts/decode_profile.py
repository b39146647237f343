#!/usr/bin/env python3
"""N replays of a Llama-3-8B decode step captured as one hipGraph, for a
kernel trace:

    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/decode_profile.py [--fp8] [--replays 20]

Without --fp8 the step is Llama.decode_native over bf16 weights, with it
LlamaFp8.decode_native over the same weights quantised (vgpu.bench.vmem's
GraphDecoder either way: two eager warm-up steps, one capture, N replays)."""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from vgpu.bench.vmem import GraphDecoder  # noqa: E402
from vgpu.models.llama import LlamaConfig  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--fp8", action="store_true")
ap.add_argument("--replays", type=int, default=20)
ap.add_argument("--ctx", type=int, default=1024)
a = ap.parse_args()
d = GraphDecoder(LlamaConfig.llama3_8b(), a.ctx, 1, native=True, fp8=a.fp8)
print(f"weights {d.weight_bytes} bytes; {d.window(a.replays)} tok/s over {a.replays} replays (under the profiler)")
torch.cuda.synchronize()
