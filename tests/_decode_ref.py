"""Shared by test_decode_cpu.py and test_gpu_decode.py: the two small Llama
configurations, their bf16-valued weights, and decode_static run step by step
on the CPU in a given precision (the reference of the decode tests)."""
import copy
import functools

import torch

from vgpu.models.llama import Llama, LlamaConfig

BF = torch.bfloat16
F64 = torch.float64
FILL = 64.0  # what unused cache rows hold: finite, and far from any k or v

CONFIGS = [
    LlamaConfig(vocab=512, dim=512, layers=2, heads=4, kv_heads=2, ffn=1024, max_seq=256),
    LlamaConfig(vocab=512, dim=1024, layers=2, heads=8, kv_heads=2, ffn=2048, max_seq=256),
]
CTX = 160
STEPS = list(range(20)) + [158, 159]  # G5's positions, in this order


@functools.lru_cache(maxsize=None)
def model(ci):
    """fp32 Llama holding bf16 values: weights N(0, 0.02), norm weights U(0.5, 1.5)."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(100 + ci)
        m = Llama(CONFIGS[ci])
        with torch.no_grad():
            for p in m.parameters():
                if p.dim() == 1:
                    p.uniform_(0.5, 1.5)
                else:
                    p.normal_(0, 0.02)
                p.copy_(p.to(BF))
    return m.eval()


def model_as(ci, dtype, device="cpu"):
    return copy.deepcopy(model(ci)).to(dtype).to(device)


@functools.lru_cache(maxsize=None)
def tokens(ci, b):
    """[len(STEPS), b, 1] token ids, one draw per (config, batch)."""
    g = torch.Generator().manual_seed(7 + 10 * ci + b)
    return torch.randint(0, CONFIGS[ci].vocab, (len(STEPS), b, 1), generator=g)


def new_cache(m, b, ctx, dtype, device="cpu"):
    cfg = m.cfg
    shape = (b, cfg.kv_heads, ctx, cfg.dim // cfg.heads)
    return [(torch.full(shape, FILL, dtype=dtype, device=device), torch.full(shape, FILL, dtype=dtype, device=device))
            for _ in range(cfg.layers)]


def run_steps(m, step, toks, kv, positions, device="cpu"):
    """`step` (a bound decode_* method) at each position; logits [len, B, vocab] as fp64 on the CPU."""
    out = []
    pos = torch.zeros(1, dtype=torch.long, device=device)
    for t, p in zip(toks, positions):
        pos.fill_(p)
        out.append(step(t.to(device), kv, pos)[:, 0].to(F64).cpu())
    return torch.stack(out)


@functools.lru_cache(maxsize=None)
def reference(ci, b):
    """fp64 and bf16 decode_static on the CPU over STEPS: logits and final caches of both."""
    toks = tokens(ci, b)
    res = {}
    for name, dtype in (("f64", F64), ("bf16", BF)):
        m = model_as(ci, dtype)
        kv = new_cache(m, b, CTX, dtype)
        res[name] = run_steps(m, m.decode_static, toks, kv, STEPS)
        res[name + "_kv"] = kv
    res["e_eager"] = (res["bf16"] - res["f64"]).abs().max().item()
    return res
