"""Shared by test_prefill_cpu.py and test_gpu_prefill.py: the inputs of the
attention cases, the fp64 causal reference with its error scale A, a pure-torch
emulation of the kernel's arithmetic class (with two deliberate mistakes to
switch on), and the CPU references of the end-to-end prefill test."""
import copy
import functools

import torch

import _decode_ref as R

BF, F64 = R.BF, R.F64
PROMPT = 37
DECODE_POS = [37, 38, 39]

# ---- P2: (B, H, KVH, hd, S, start, ctx) ---------------------------------------------------
S_AT_ZERO = [1, 15, 16, 17, 33, 63, 64, 65, 127, 129, 257]
CONTINUED = [(1, 70), (5, 59), (67, 61), (64, 64), (33, 255)]
HEADS = [(4, 2), (8, 2)]
P2_CASES = [(B, H, KVH, hd, S, start, start + S + 5)
            for hd in (64, 128) for H, KVH in HEADS for B in (1, 2)
            for S, start in [(s, 0) for s in S_AT_ZERO] + CONTINUED]
# G = 8 and G = 1
P2_CASES += [(1, H, KVH, hd, S, start, start + S + 5)
             for hd in (64, 128) for H, KVH in [(8, 1), (2, 2)] for S, start in [(65, 0), (67, 61)]]
# the cache ends exactly at the last prompt token
P2_CASES += [(2, 4, 2, 128, 67, 61, 128), (1, 8, 2, 64, 129, 0, 129)]
PREFIX_CASES = [(1, 4, 2, 128, 129, 0, 134), (2, 8, 2, 64, 129, 0, 134), (1, 8, 2, 128, 67, 61, 133),
                (2, 4, 2, 64, 67, 61, 133)]


def case_id(case):
    return "B{}-H{}-KVH{}-hd{}-S{}-start{}-ctx{}".format(*case)


@functools.lru_cache(maxsize=None)
def p2_inputs(case):
    """q [B, S, H, hd], k / v [B, KVH, ctx, hd] bf16 (rows >= start + S hold 64.0), scale."""
    B, H, KVH, hd, S, start, ctx = case
    g = torch.Generator().manual_seed(sum(p * c for p, c in zip((3, 5, 7, 11, 13, 17, 19), case)))
    q = torch.randn(B, S, H, hd, generator=g).to(BF)
    k = torch.randn(B, KVH, ctx, hd, generator=g).to(BF)
    v = torch.randn(B, KVH, ctx, hd, generator=g).to(BF)
    k[:, :, start + S:] = R.FILL
    v[:, :, start + S:] = R.FILL
    return q, k, v, hd ** -0.5


def attn64(q, k, v, start, scale):
    """fp64 causal attention from the bf16 values: row i of head h over cache
    rows 0 .. start + i of kv head h // (H / KVH).  Returns (ref, A), both
    [B, S, H, hd]: A is the same softmax weights applied to |v|."""
    B, S, H, hd = q.shape
    rep = H // k.shape[1]
    n = start + S
    k64 = k[:, :, :n].to(F64).repeat_interleave(rep, dim=1)
    v64 = v[:, :, :n].to(F64).repeat_interleave(rep, dim=1)
    s = torch.einsum("bshd,bhkd->bhsk", q.to(F64), k64) * scale
    allowed = torch.arange(n)[None, :] <= (start + torch.arange(S))[:, None]
    w = torch.softmax(s.masked_fill(~allowed, float("-inf")), dim=-1)
    ref = torch.einsum("bhsk,bhkd->bshd", w, v64)
    return ref, torch.einsum("bhsk,bhkd->bshd", w, v64.abs())


def emulate(q, k, v, start, scale, mask_shift=0, wrong_gqa=False, tile=64):
    """The kernel's arithmetic class in torch: fp32 scores from the bf16
    values, keys in tiles of 64, online softmax with fp32 m and l, P rounded to
    bf16 into the PV product, fp32 accumulation, one rounding of the output to
    bf16.  mask_shift = +1 / -1 lets row i see one key more / fewer;
    wrong_gqa maps query head h to kv head h % KVH.  Keys are read up to the
    end of the cache if the mask asks for them (the 64.0 fill)."""
    B, S, H, hd = q.shape
    KVH, ctx = k.shape[1], k.shape[2]
    heads = torch.arange(H) % KVH if wrong_gqa else torch.arange(H) // (H // KVH)
    qf = q.float().permute(0, 2, 1, 3)                     # [B, H, S, hd]
    kf, vf = k.float()[:, heads], v.float()[:, heads]      # [B, H, ctx, hd]
    last = start + torch.arange(S) + mask_shift            # the last key each row sees
    n = min(ctx, int(last.max()) + 1)
    m = torch.full((B, H, S), float("-inf"))
    l = torch.zeros(B, H, S)
    o = torch.zeros(B, H, S, hd)
    for k0 in range(0, n, tile):
        k1 = min(k0 + tile, n)
        s = torch.matmul(qf, kf[:, :, k0:k1].transpose(-1, -2)) * scale
        allowed = torch.arange(k0, k1)[None, :] <= last[:, None]
        s = s.masked_fill(~allowed, float("-inf"))
        mx = torch.maximum(m, s.amax(dim=-1))
        safe = torch.where(mx == float("-inf"), torch.zeros_like(mx), mx)  # -inf - -inf: nothing seen yet
        alpha = torch.exp(m - safe)
        p = torch.exp(s - safe[..., None])
        l = l * alpha + p.sum(dim=-1)
        o = o * alpha[..., None] + torch.matmul(p.to(BF).float(), vf[:, :, k0:k1])
        m = mx
    out = torch.where(l[..., None] > 0, o / l[..., None].clamp_min(1e-30), torch.zeros_like(o))
    return out.to(BF).permute(0, 2, 1, 3).contiguous()     # [B, S, H, hd]


def excess(got, ref, A):
    """max over elements of |got - ref| / (2^-7 A): at most 1 inside P2's bound."""
    return ((got.to(F64) - ref).abs() / (2.0 ** -7 * A)).max().item()


# ---- P4: the prompt, the decode tokens after it, and both CPU runs ------------------------

@functools.lru_cache(maxsize=None)
def p4_tokens(ci, b):
    """([b, 37] prompt, [3, b, 1] tokens of the decode steps after it), one generator per (config, batch)."""
    g = torch.Generator().manual_seed(900 + 10 * ci + b)
    vocab = R.CONFIGS[ci].vocab
    return torch.randint(0, vocab, (b, PROMPT), generator=g), torch.randint(0, vocab, (3, b, 1), generator=g)


@functools.lru_cache(maxsize=None)
def p4_reference(ci, b):
    """forward(tokens, kv, 0) and three decode_static steps after it on the CPU,
    in fp64 and in bf16: logits (fp64 tensors), the caches right after the
    prompt, and the eager run's largest logit errors."""
    prompt, dec = p4_tokens(ci, b)
    res = {}
    for name, dtype in (("f64", F64), ("bf16", BF)):
        m = R.model_as(ci, dtype)
        kv = R.new_cache(m, b, R.CTX, dtype)
        with torch.no_grad():
            res[name] = m(prompt, kv, 0)[:, 0].to(F64)
        res[name + "_kv"] = copy.deepcopy(kv)
        res[name + "_dec"] = R.run_steps(m, m.decode_static, dec, kv, DECODE_POS)
    res["e_eager"] = (res["bf16"] - res["f64"]).abs().max().item()
    res["e_eager_dec"] = (res["bf16_dec"] - res["f64_dec"]).abs().max().item()
    return res
