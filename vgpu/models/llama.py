"""Llama-3 decoder (random init) for the virtual-device-memory workload
(BASELINE.json config 5: "one pod requests gpumem=400000M on a 288 GB MI355X,
Llama-3-8B random-init inference via host-swap paging").

Standard architecture: RMSNorm, RoPE (theta 500k), grouped-query attention
through F.scaled_dot_product_attention (flash/CK path on ROCm), SwiGLU MLP,
untied embeddings.  `LlamaConfig.llama3_8b()` is the 8B shape; tests use
`LlamaConfig.tiny()`.
"""
from __future__ import annotations

from dataclasses import dataclass

import torch
from torch import nn
import torch.nn.functional as F


@dataclass
class LlamaConfig:
    vocab: int = 128256
    dim: int = 4096
    layers: int = 32
    heads: int = 32
    kv_heads: int = 8
    ffn: int = 14336
    rope_theta: float = 500000.0
    max_seq: int = 8192
    eps: float = 1e-5

    @staticmethod
    def llama3_8b() -> "LlamaConfig":
        return LlamaConfig()

    @staticmethod
    def tiny() -> "LlamaConfig":
        return LlamaConfig(vocab=512, dim=128, layers=2, heads=4, kv_heads=2, ffn=256, max_seq=256)


class RMSNorm(nn.Module):
    def __init__(self, dim: int, eps: float):
        super().__init__()
        self.weight = nn.Parameter(torch.ones(dim))
        self.eps = eps

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        xf = x.float()
        y = xf * torch.rsqrt(xf.pow(2).mean(-1, keepdim=True) + self.eps)
        return (y * self.weight.float()).to(x.dtype)


def rope_tables(cfg: LlamaConfig, device=None) -> tuple[torch.Tensor, torch.Tensor]:
    hd = cfg.dim // cfg.heads
    inv = 1.0 / (cfg.rope_theta ** (torch.arange(0, hd, 2, device=device).float() / hd))
    t = torch.arange(cfg.max_seq, device=device).float()
    f = torch.outer(t, inv)
    return f.cos(), f.sin()


def apply_rope(x: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor) -> torch.Tensor:
    # x: [B, H, S, D]; cos/sin: [S, D/2]
    x1, x2 = x.float().chunk(2, dim=-1)
    c, s = cos[None, None], sin[None, None]
    return torch.cat([x1 * c - x2 * s, x1 * s + x2 * c], dim=-1).to(x.dtype)


class Attention(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.h, self.kvh, self.hd = cfg.heads, cfg.kv_heads, cfg.dim // cfg.heads
        self.wqkv = nn.Linear(cfg.dim, (cfg.heads + 2 * cfg.kv_heads) * self.hd, bias=False)
        self.wo = nn.Linear(cfg.dim, cfg.dim, bias=False)

    def forward(self, x, cos, sin, kv_cache=None, pos: int = 0):
        B, S, _ = x.shape
        qkv = self.wqkv(x)
        q, k, v = qkv.split([self.h * self.hd, self.kvh * self.hd, self.kvh * self.hd], dim=-1)
        q = q.view(B, S, self.h, self.hd).transpose(1, 2)
        k = k.view(B, S, self.kvh, self.hd).transpose(1, 2)
        v = v.view(B, S, self.kvh, self.hd).transpose(1, 2)
        q = apply_rope(q, cos[pos:pos + S], sin[pos:pos + S])
        k = apply_rope(k, cos[pos:pos + S], sin[pos:pos + S])
        if kv_cache is not None:
            kc, vc = kv_cache
            kc[:, :, pos:pos + S] = k
            vc[:, :, pos:pos + S] = v
            k, v = kc[:, :, :pos + S], vc[:, :, :pos + S]
        rep = self.h // self.kvh
        if rep > 1:
            k = k.repeat_interleave(rep, dim=1)
            v = v.repeat_interleave(rep, dim=1)
        o = F.scaled_dot_product_attention(q, k, v, is_causal=(S > 1))
        return self.wo(o.transpose(1, 2).reshape(B, S, -1))


class Block(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.norm1 = RMSNorm(cfg.dim, cfg.eps)
        self.attn = Attention(cfg)
        self.norm2 = RMSNorm(cfg.dim, cfg.eps)
        self.w13 = nn.Linear(cfg.dim, 2 * cfg.ffn, bias=False)
        self.w2 = nn.Linear(cfg.ffn, cfg.dim, bias=False)

    def forward(self, x, cos, sin, kv_cache=None, pos: int = 0):
        x = x + self.attn(self.norm1(x), cos, sin, kv_cache, pos)
        g, u = self.w13(self.norm2(x)).chunk(2, dim=-1)
        return x + self.w2(F.silu(g) * u)


LINEARS = ("wqkv", "wo", "w13", "w2")  # the projections of a layer, in the order a step applies them


def _decode_step(cfg, x, norms, norm_f, rope, kv_caches, pos, linear):
    """The body of a native decode step (vgpu.ops.decode), shared by Llama and
    LlamaFp8.  x: the embedded tokens [B, 1, dim]; norms: per layer (norm1,
    norm2) weights; `linear(name, i, x, y)` applies projection `name` (one of
    LINEARS, or "head" with i None) of layer i to x [B, K] into y [B, N]: the
    one thing the two models do differently."""
    from vgpu.ops import decode as D
    B, dev = x.shape[0], x.device
    H, KVH, hd = cfg.heads, cfg.kv_heads, cfg.dim // cfg.heads
    ctx = kv_caches[0][0].shape[2] if kv_caches else 1
    cos, sin = rope

    def buf(*shape, dtype=torch.bfloat16):
        return torch.empty(shape, dtype=dtype, device=dev)

    x = x.view(B, cfg.dim)  # the residual stream, updated in place
    h, qkv, q = buf(B, cfg.dim), buf(B, (H + 2 * KVH) * hd), buf(B, H, hd)
    att, ao, mlp = buf(B, H * hd), buf(B, cfg.dim), buf(B, cfg.dim)
    gu, act = buf(B, 2 * cfg.ffn), buf(B, cfg.ffn)
    ws = buf(D.attn_workspace_bytes(B, H, hd, ctx) // 4, dtype=torch.float32)
    scale = hd ** -0.5
    delta = None
    for i, ((norm1, norm2), (kc, vc)) in enumerate(zip(norms, kv_caches)):
        D.add_rmsnorm(x, delta, norm1, h, cfg.eps)
        linear("wqkv", i, h, qkv)
        D.rope_kv_write(qkv, cos, sin, pos, q, kc, vc)
        D.attn_decode(q, kc, vc, pos, att, ws, scale)
        linear("wo", i, att, ao)
        D.add_rmsnorm(x, ao, norm2, h, cfg.eps)
        linear("w13", i, h, gu)
        D.swiglu(gu, act)
        linear("w2", i, act, mlp)
        delta = mlp
    D.add_rmsnorm(x, delta, norm_f, h, cfg.eps)
    logits = buf(B, cfg.vocab)
    linear("head", None, h, logits)
    return logits.view(B, 1, cfg.vocab)


def _prefill(cfg, x, norms, norm_f, rope, kv_caches, start, linear):
    """The body of a native prompt pass (vgpu.ops.prefill), shared by Llama and
    LlamaFp8; arguments as _decode_step's, x [B, S, dim].  "head" gets each
    sequence's last row only, [B, dim]."""
    from vgpu.ops import decode as D, prefill as P
    (B, S), dev = x.shape[:2], x.device
    H, KVH, hd = cfg.heads, cfg.kv_heads, cfg.dim // cfg.heads
    rows = B * S
    cos, sin = rope

    def buf(*shape):
        return torch.empty(shape, dtype=torch.bfloat16, device=dev)

    x = x.view(rows, cfg.dim)  # the residual stream, updated in place
    h, qkv, q = buf(rows, cfg.dim), buf(rows, (H + 2 * KVH) * hd), buf(B, S, H, hd)
    att, ao, mlp = buf(B, S, H * hd), buf(rows, cfg.dim), buf(rows, cfg.dim)
    gu, act = buf(rows, 2 * cfg.ffn), buf(rows, cfg.ffn)
    scale = hd ** -0.5
    delta = None
    for i, ((norm1, norm2), (kc, vc)) in enumerate(zip(norms, kv_caches)):
        D.add_rmsnorm(x, delta, norm1, h, cfg.eps)
        linear("wqkv", i, h, qkv)
        P.rope_kv_write_seq(qkv, cos, sin, start, q, kc, vc)
        P.attn_prefill(q, kc, vc, start, att, scale)
        linear("wo", i, att.view(rows, H * hd), ao)
        D.add_rmsnorm(x, ao, norm2, h, cfg.eps)
        linear("w13", i, h, gu)
        D.swiglu(gu, act)
        linear("w2", i, act, mlp)
        delta = mlp
    # only each sequence's last row goes through the final norm and the head
    xl = x.view(B, S, cfg.dim)[:, -1].contiguous()
    dl = delta.view(B, S, cfg.dim)[:, -1].contiguous() if delta is not None else None
    hl, logits = buf(B, cfg.dim), buf(B, cfg.vocab)
    D.add_rmsnorm(xl, dl, norm_f, hl, cfg.eps)
    linear("head", None, hl, logits)
    return logits.view(B, 1, cfg.vocab)


@torch.no_grad()
def _generate(model, tokens, kv_caches, max_new, start, temperature, top_k, top_p, seed, eos, graph):
    """The body of generate_native, shared by Llama and LlamaFp8: the model's
    own prefill_native and decode_native with vgpu.ops.select after each."""
    from vgpu.ops import select as S
    cfg = model.cfg
    if tokens.dim() != 2 or tokens.shape[1] < 1:
        raise ValueError(f"tokens: shape {tuple(tokens.shape)}, expected [B, S] with S >= 1")
    B, S_ = tokens.shape
    greedy = temperature == 0
    why = S.shape_reason(B, cfg.vocab, 1 if greedy else top_k)
    if not why and not greedy:
        why = S.params_reason(temperature, top_k, top_p)
    if why:
        raise ValueError(f"generate not supported: {why}")
    if not isinstance(max_new, int) or max_new < 1:
        raise ValueError(f"max_new: {max_new!r}, expected an integer >= 1")
    if len(kv_caches) != cfg.layers or not cfg.layers or kv_caches[0][0].dim() != 4:
        raise ValueError(f"kv_caches: expected {cfg.layers} layers of [B, KVH, ctx, hd] pairs")
    limit = min(kv_caches[0][0].shape[2], cfg.max_seq)
    if start < 0 or start + S_ + max_new - 1 > limit:
        raise ValueError(f"start {start} + prompt {S_} + max_new {max_new} - 1 exceeds min(ctx, max_seq) = {limit}")
    eos = -1 if eos is None else eos
    if not isinstance(eos, int) or not -1 <= eos < cfg.vocab:
        raise ValueError(f"eos: {eos!r}, expected None or a token id below {cfg.vocab}")
    dev = tokens.device
    out = torch.zeros(B, max_new, dtype=torch.int64, device=dev)
    next_tok = torch.zeros(B, 1, dtype=torch.int64, device=dev)
    step = torch.zeros(1, dtype=torch.int64, device=dev)
    pos = torch.full((1,), start + S_ - 1, dtype=torch.int64, device=dev)
    u = None
    if not greedy:  # drawn on the CPU, copied once: a run is a function of its arguments
        u = torch.rand(max_new, B, generator=torch.Generator().manual_seed(seed)).to(dev)

    logits = model.prefill_native(tokens, kv_caches, start)
    ws = torch.empty(S.workspace_bytes(B, cfg.vocab) // 4, dtype=torch.int32, device=dev)

    def select(logits):
        lg = logits.view(B, cfg.vocab)
        if greedy:
            S.greedy(lg, ws, step, pos, next_tok, out, eos)
        else:
            S.sample(lg, ws, step, pos, next_tok, out, u, temperature, top_k, top_p, eos)

    def decode_select():
        select(model.decode_native(next_tok, kv_caches, pos))

    select(logits)  # pos: now the row the new token's k / v go to
    left = max_new - 1
    if graph and max_new > 2:
        decode_select()  # eager: real work, and it loads every kernel
        left -= 1
        g = torch.cuda.CUDAGraph()
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.graph(g, stream=side):  # a capture executes nothing: no state to restore
            decode_select()
        for _ in range(left):
            g.replay()
    else:
        for _ in range(left):
            decode_select()
    torch.cuda.current_stream().synchronize()
    return out


class Llama(nn.Module):
    def __init__(self, cfg: LlamaConfig):
        super().__init__()
        self.cfg = cfg
        self.embed = nn.Embedding(cfg.vocab, cfg.dim)
        self.layers = nn.ModuleList([Block(cfg) for _ in range(cfg.layers)])
        self.norm = RMSNorm(cfg.dim, cfg.eps)
        self.head = nn.Linear(cfg.dim, cfg.vocab, bias=False)
        self._rope = None

    def rope(self, device):
        if self._rope is None or self._rope[0].device != device:
            self._rope = rope_tables(self.cfg, device)
        return self._rope

    def _linear(self, name, i) -> nn.Linear:
        """Projection `name` (one of LINEARS) of layer i, or the head (i None)."""
        if name == "head":
            return self.head
        layer = self.layers[i]
        return getattr(layer.attn if name in ("wqkv", "wo") else layer, name)

    def forward(self, tokens: torch.Tensor, kv_caches=None, pos: int = 0) -> torch.Tensor:
        cos, sin = self.rope(tokens.device)
        x = self.embed(tokens)
        for i, layer in enumerate(self.layers):
            x = layer(x, cos, sin, kv_caches[i] if kv_caches is not None else None, pos)
        return self.head(self.norm(x[:, -1:]))

    @torch.no_grad()
    def decode_static(self, tokens: torch.Tensor, kv_caches, pos: torch.Tensor) -> torch.Tensor:
        """One decode step with every shape fixed (graph-capturable): `pos` is
        a 1-element device tensor, the cache is written with index_copy_ and
        attention runs over the whole cache with positions > pos masked."""
        cos, sin = self.rope(tokens.device)
        c, s_ = cos.index_select(0, pos), sin.index_select(0, pos)
        x = self.embed(tokens)
        B = x.shape[0]
        ctx = kv_caches[0][0].shape[2]
        mask = (torch.arange(ctx, device=tokens.device) <= pos)[None, None, None, :]
        for i, layer in enumerate(self.layers):
            a = layer.attn
            h = layer.norm1(x)
            q, k, v = a.wqkv(h).split([a.h * a.hd, a.kvh * a.hd, a.kvh * a.hd], dim=-1)
            q = apply_rope(q.view(B, 1, a.h, a.hd).transpose(1, 2), c, s_)
            k = apply_rope(k.view(B, 1, a.kvh, a.hd).transpose(1, 2), c, s_)
            v = v.view(B, 1, a.kvh, a.hd).transpose(1, 2)
            kc, vc = kv_caches[i]
            kc.index_copy_(2, pos, k)
            vc.index_copy_(2, pos, v)
            rep = a.h // a.kvh
            kk = kc.repeat_interleave(rep, dim=1) if rep > 1 else kc
            vv = vc.repeat_interleave(rep, dim=1) if rep > 1 else vc
            o = F.scaled_dot_product_attention(q, kk, vv, attn_mask=mask)
            x = x + a.wo(o.transpose(1, 2).reshape(B, 1, -1))
            g, u = layer.w13(layer.norm2(x)).chunk(2, dim=-1)
            x = x + layer.w2(F.silu(g) * u)
        return self.head(self.norm(x))

    @torch.no_grad()
    def decode_native(self, tokens: torch.Tensor, kv_caches, pos: torch.Tensor) -> torch.Tensor:
        """decode_static on the native kernels (vgpu.ops.decode): ten
        dispatches per layer, K / V read in place for grouped-query attention,
        `pos` read on the device (graph-capturable).  bf16 weights and
        contiguous bf16 caches on the GPU, batch 1-4 or 8, head_dim 64 or 128;
        anything else raises ValueError."""
        from vgpu.ops import decode as D
        D.check_llama(self, tokens, kv_caches, pos, prefill=False, fp8=False)

        def linear(name, i, x, y):
            D.gemv(x, self._linear(name, i).weight, y)

        return _decode_step(self.cfg, self.embed(tokens), [(l.norm1.weight, l.norm2.weight) for l in self.layers],
                            self.norm.weight, self.rope(tokens.device), kv_caches, pos, linear)

    @torch.no_grad()
    def prefill_native(self, tokens: torch.Tensor, kv_caches, start: int = 0) -> torch.Tensor:
        """`forward(tokens [B, S], kv_caches, start)` on the native kernels
        (vgpu.ops.prefill): the projections on the bf16 MFMA GEMM, RoPE and
        the cache write for all S tokens in one launch, causal grouped-query
        flash attention reading K / V in place.  Writes cache rows start ..
        start + S - 1 and attends to rows 0 .. start + i, so a prompt may come
        in chunks; `start` is a host int (not graph-replayable at another
        position).  bf16 weights and contiguous bf16 caches on the GPU,
        head_dim 64 or 128, dim / ffn / qkv width / vocab multiples of 64;
        anything else raises ValueError.  Returns the last token's logits
        [B, 1, vocab]."""
        from vgpu.ops import decode as D, prefill as P
        D.check_llama(self, tokens, kv_caches, start, prefill=True, fp8=False)

        def linear(name, i, x, y):
            # the head has B rows: the GEMV where it takes the batch
            gemv = name == "head" and x.shape[0] in D.BATCHES
            (D.gemv if gemv else P.gemm)(x, self._linear(name, i).weight, y)

        return _prefill(self.cfg, self.embed(tokens), [(l.norm1.weight, l.norm2.weight) for l in self.layers],
                        self.norm.weight, self.rope(tokens.device), kv_caches, start, linear)

    def generate_native(self, tokens: torch.Tensor, kv_caches, max_new: int, *, start: int = 0,
                        temperature: float = 0.0, top_k: int = 1, top_p: float = 1.0, seed: int = 0, eos=None,
                        graph: bool = True) -> torch.Tensor:
        """`max_new` tokens after the prompt `tokens` [B, S] (int64), chosen on the
        device: prefill_native, then decode_native max_new - 1 times, each followed
        by vgpu.ops.select, which writes the token where the next embedding reads
        it and advances `pos` there.  temperature 0: greedy (first index in
        select's ordering); otherwise top-k (at most 64) / top-p sampling at that
        temperature, with u = torch.rand(max_new, B, generator=torch.Generator()
        .manual_seed(seed)) drawn on the CPU, so a run is reproducible from its
        arguments.  top_p acts inside the top-k set only (no nucleus over the whole
        vocabulary).  graph (and max_new > 2): the first decode + select runs
        eagerly, the second is captured as one graph on a side stream and
        replayed for the rest with no host work between replays.  One host
        synchronisation, at the end.  With `eos` the loop still runs max_new steps:
        a row that has emitted eos is padded with eos.  Needs max_new >= 1 and
        start + S + max_new - 1 <= min(ctx, cfg.max_seq) (the last token chosen is
        never fed back); otherwise, and for whatever prefill_native, decode_native
        or select refuse, ValueError.  Returns int64 [B, max_new]."""
        return _generate(self, tokens, kv_caches, max_new, start, temperature, top_k, top_p, seed, eos, graph)

    def new_kv_cache(self, batch: int, seq: int, dtype=torch.bfloat16, device=None):
        hd = self.cfg.dim // self.cfg.heads
        shape = (batch, self.cfg.kv_heads, seq, hd)
        return [(torch.empty(shape, dtype=dtype, device=device),
                 torch.empty(shape, dtype=dtype, device=device)) for _ in range(self.cfg.layers)]


class Fp8Linear(nn.Module):
    """A bias-free Linear's weight [N, K] as e4m3fn codes and one fp32 scale per row (vgpu.ops.fp8)."""

    def __init__(self, codes: torch.Tensor, scale: torch.Tensor):
        super().__init__()
        self.register_buffer("codes", codes)
        self.register_buffer("scale", scale)


class Fp8Block(nn.Module):
    def __init__(self, norm1, norm2, **linears):
        super().__init__()
        self.register_buffer("norm1", norm1)
        self.register_buffer("norm2", norm2)
        for name in LINEARS:
            setattr(self, name, linears[name])


class LlamaFp8(nn.Module):
    """A Llama whose projection weights (wqkv, wo, w13, w2 of every layer, and
    the head) are held in fp8: half the bytes a decode step streams and half the
    HBM of the projections.  The embedding and the norm weights stay bf16.
    Inference on the native kernels only; everything is a buffer."""

    def __init__(self, cfg: LlamaConfig, embed, layers, norm, head):
        super().__init__()
        self.cfg = cfg
        self.register_buffer("embed", embed)
        self.layers = nn.ModuleList(layers)
        self.register_buffer("norm", norm)
        self.head = head
        self._rope = None

    rope = Llama.rope
    new_kv_cache = Llama.new_kv_cache
    generate_native = Llama.generate_native  # over this class's prefill_native and decode_native

    @classmethod
    @torch.no_grad()
    def from_llama(cls, model: Llama, device=None) -> "LlamaFp8":
        """Quantise `model` (on the CPU or the GPU, any floating dtype) one
        Linear at a time, each on the device it sits on, and place the result on
        `device` (None: where the model is): beyond the result, one weight's
        worth of memory at the peak."""
        from vgpu.ops import fp8 as Q
        if not isinstance(model, Llama):
            raise ValueError(f"model: {type(model).__name__}, expected a Llama")
        Q.check_llama_fp8_config(model.cfg)

        def keep(t):
            return t.detach().to(device=device, dtype=torch.bfloat16).contiguous()

        def lin(m, name):
            try:
                codes, scale = Q.quantize(m.weight)
            except ValueError as e:
                raise ValueError(f"{name}: {e}") from None
            return Fp8Linear(codes.to(device), scale.to(device))

        layers = []
        for i, l in enumerate(model.layers):
            layers.append(Fp8Block(keep(l.norm1.weight), keep(l.norm2.weight),
                                   **{n: lin(model._linear(n, i), f"layers.{i}.{n}") for n in LINEARS}))
        return cls(model.cfg, keep(model.embed.weight), layers, keep(model.norm.weight), lin(model.head, "head")).eval()

    @torch.no_grad()
    def dequantized(self) -> Llama:
        """A bf16 Llama (on this model's device) holding exactly the values this model represents."""
        from vgpu.ops import fp8 as Q
        with torch.device("meta"):
            m = Llama(self.cfg)
        m = m.to(torch.bfloat16).to_empty(device=self.embed.device)
        m.embed.weight.copy_(self.embed)
        m.norm.weight.copy_(self.norm)
        for src, dst in zip(self.layers, m.layers):
            dst.norm1.weight.copy_(src.norm1)
            dst.norm2.weight.copy_(src.norm2)
        for name, i in [("head", None)] + [(name, i) for i in range(self.cfg.layers) for name in LINEARS]:
            q = self._linear(name, i)
            m._linear(name, i).weight.copy_(Q.dequantize_ref(q.codes, q.scale))
        return m.eval()

    def _linear(self, name, i) -> Fp8Linear:
        return self.head if name == "head" else getattr(self.layers[i], name)

    def _norms(self):
        return [(l.norm1, l.norm2) for l in self.layers]

    @torch.no_grad()
    def decode_native(self, tokens: torch.Tensor, kv_caches, pos: torch.Tensor) -> torch.Tensor:
        """Llama.decode_native with the fp8 GEMV (vgpu.ops.fp8.gemv_fp8) in place
        of the bf16 one: the same ten dispatches per layer, the same caches,
        `pos` read on the device (graph-capturable)."""
        from vgpu.ops import decode as D, fp8 as Q
        D.check_llama(self, tokens, kv_caches, pos, prefill=False, fp8=True)

        def linear(name, i, x, y):
            q = self._linear(name, i)
            Q.gemv_fp8(x, q.codes, q.scale, y)

        return _decode_step(self.cfg, F.embedding(tokens, self.embed), self._norms(), self.norm,
                            self.rope(tokens.device), kv_caches, pos, linear)

    @torch.no_grad()
    def prefill_native(self, tokens: torch.Tensor, kv_caches, start: int = 0) -> torch.Tensor:
        """Llama.prefill_native over the fp8 weights: each projection's weight is
        expanded to bf16 (vgpu.ops.fp8.dequant) into one scratch buffer, sized
        for the largest weight and allocated once per call, and fed to the bf16
        MFMA GEMM.  With power-of-two scales this is `dequantized()
        .prefill_native` bit for bit.  The head takes the fp8 GEMV where that
        takes the batch."""
        from vgpu.ops import decode as D, fp8 as Q, prefill as P
        D.check_llama(self, tokens, kv_caches, start, prefill=True, fp8=True)
        cfg = self.cfg
        B = tokens.shape[0]
        largest = max([getattr(l, name).codes.numel() for l in self.layers for name in LINEARS]
                      + [0 if B in D.BATCHES else self.head.codes.numel()])
        scratch = torch.empty(largest, dtype=torch.bfloat16, device=tokens.device)

        def linear(name, i, x, y):
            q = self._linear(name, i)
            if name == "head" and B in D.BATCHES:
                Q.gemv_fp8(x, q.codes, q.scale, y)
                return
            w = scratch[:q.codes.numel()].view(q.codes.shape)
            Q.dequant(q.codes, q.scale, w)
            P.gemm(x, w, y)

        return _prefill(cfg, F.embedding(tokens, self.embed), self._norms(), self.norm, self.rope(tokens.device),
                        kv_caches, start, linear)

