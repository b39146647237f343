"""One Llama decode step on the native kernels (native/kernels/decode.hip and
the forward GEMV of skinny.hip): residual add + RMSNorm, RoPE + KV-cache write,
grouped-query attention over the cache without repeating K / V, SwiGLU.

Every function writes into buffers the caller owns and reads `pos` on the
device, so a sequence of them captures into one graph.  Arguments are checked
here, before the library is loaded; a tensor the kernels cannot take raises
ValueError naming the reason (never a fall-back to eager)."""
from __future__ import annotations

import ctypes

import torch

from vgpu.native import load_kernels

BF16 = torch.bfloat16
BATCHES = (1, 2, 3, 4, 8)
HEAD_DIMS = (64, 128)
MAX_GROUP = 8  # query heads per kv head
_BOUND = False


def _lib():
    global _BOUND
    lib = load_kernels()
    if not _BOUND:
        vp, ci, i64, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
        lib.vgpu_decode_supported.argtypes = [ci] * 5
        lib.vgpu_decode_supported.restype = ci
        lib.vgpu_add_rmsnorm.argtypes = [vp] * 4 + [ci, ci, cf, vp]
        lib.vgpu_add_rmsnorm.restype = ci
        lib.vgpu_rope_kv_write.argtypes = [vp] * 7 + [ci] * 6 + [vp]
        lib.vgpu_rope_kv_write.restype = ci
        lib.vgpu_attn_decode_chunk.argtypes = [ci]
        lib.vgpu_attn_decode_chunk.restype = ci
        lib.vgpu_attn_decode_workspace.argtypes = [ci] * 4
        lib.vgpu_attn_decode_workspace.restype = i64
        lib.vgpu_attn_decode.argtypes = [vp] * 6 + [i64] + [ci] * 5 + [cf, vp]
        lib.vgpu_attn_decode.restype = ci
        lib.vgpu_swiglu.argtypes = [vp, vp, ci, ci, vp]
        lib.vgpu_swiglu.restype = ci
        lib.vgpu_skinny_fwd.argtypes = [vp] * 4 + [ci] * 4 + [vp]
        lib.vgpu_skinny_fwd.restype = ci
        _BOUND = True
    return lib


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what}: error {rc}")


# ---- argument checks (no library, no device needed) -------------------------------------

def shape_reason(B: int, H: int, KVH: int, hd: int, ctx: int) -> str | None:
    """Why vgpu_decode_supported refuses this shape (None: it takes it)."""
    if B not in BATCHES:
        return f"batch {B} not in {BATCHES}"
    if hd not in HEAD_DIMS:
        return f"head_dim {hd} not in {HEAD_DIMS}"
    if H < 1 or KVH < 1 or H % KVH:
        return f"heads {H} not a multiple of kv_heads {KVH}"
    if H // KVH > MAX_GROUP:
        return f"{H // KVH} query heads per kv head (at most {MAX_GROUP})"
    if ctx < 1:
        return f"context {ctx} < 1"
    return None


def _want(t: torch.Tensor, name: str, shape, dtype=BF16, device: bool = True) -> None:
    """Shape, then layout, then dtype, then device: the reason named is the
    first that holds on any machine."""
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    if not t.is_contiguous():
        raise ValueError(f"{name}: not contiguous (strides {t.stride()})")
    if t.dtype != dtype:
        raise ValueError(f"{name}: dtype {t.dtype}, expected {dtype}")
    if device and not t.is_cuda:
        raise ValueError(f"{name}: on {t.device}, expected a GPU tensor")


def _want_pos(pos: torch.Tensor) -> None:
    _want(pos, "pos", (1,), torch.int64)


def _want_shape(B, H, KVH, hd, ctx) -> None:
    why = shape_reason(B, H, KVH, hd, ctx)
    if why:
        raise ValueError(f"decode shape not supported: {why}")


# ---- the kernels -----------------------------------------------------------------------

def add_rmsnorm(x: torch.Tensor, delta: torch.Tensor | None, w: torch.Tensor, y: torch.Tensor, eps: float) -> None:
    """x [rows, dim] += delta in place (delta None: x as it is); y = RMSNorm(x) * w."""
    if x.dim() != 2 or x.shape[1] % 8 or x.shape[1] < 8 or x.shape[0] < 1:
        raise ValueError(f"x: shape {tuple(x.shape)}, expected [rows, dim] with dim % 8 == 0")
    rows, dim = x.shape
    _want(x, "x", (rows, dim))
    if delta is not None:
        _want(delta, "delta", (rows, dim))
    _want(w, "w", (dim,))
    _want(y, "y", (rows, dim))
    _check(_lib().vgpu_add_rmsnorm(_p(x), _p(delta), _p(w), _p(y), rows, dim, float(eps), _stream()),
           "vgpu_add_rmsnorm")


def rope_kv_write(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, pos: torch.Tensor, q_out: torch.Tensor,
                  kcache: torch.Tensor, vcache: torch.Tensor) -> None:
    """qkv [B, (H + 2 KVH) hd] -> rotated q into q_out [B, H, hd], rotated k and
    raw v into row `pos` of the [B, KVH, ctx, hd] caches.  cos / sin are
    rope_tables' [max_seq, hd / 2] fp32."""
    if q_out.dim() != 3 or kcache.dim() != 4:
        raise ValueError(f"q_out / kcache: shapes {tuple(q_out.shape)} / {tuple(kcache.shape)}, expected "
                         "[B, H, hd] / [B, KVH, ctx, hd]")
    B, H, hd = q_out.shape
    KVH, ctx = kcache.shape[1], kcache.shape[2]
    _want_shape(B, H, KVH, hd, ctx)
    if cos.dim() != 2 or cos.shape[0] < 1:
        raise ValueError(f"cos: shape {tuple(cos.shape)}, expected [max_seq, {hd // 2}]")
    max_seq = cos.shape[0]
    _want(qkv, "qkv", (B, (H + 2 * KVH) * hd))
    _want(cos, "cos", (max_seq, hd // 2), torch.float32)
    _want(sin, "sin", (max_seq, hd // 2), torch.float32)
    _want_pos(pos)
    _want(q_out, "q_out", (B, H, hd))
    _want(kcache, "kcache", (B, KVH, ctx, hd))
    _want(vcache, "vcache", (B, KVH, ctx, hd))
    _check(_lib().vgpu_rope_kv_write(_p(qkv), _p(cos), _p(sin), _p(pos), _p(q_out), _p(kcache), _p(vcache), B, H, KVH,
                                     hd, ctx, max_seq, _stream()), "vgpu_rope_kv_write")


def attn_workspace_bytes(B: int, H: int, hd: int, ctx: int) -> int:
    _want_shape(B, H, H, hd, ctx)
    return int(_lib().vgpu_attn_decode_workspace(B, H, hd, ctx))


def attn_decode(q: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor, pos: torch.Tensor, out: torch.Tensor,
                ws: torch.Tensor, scale: float) -> None:
    """out [B, H hd] = softmax(q K^T scale) V over cache rows 0..pos, query head
    h reading kv head h // (H / KVH).  ws: fp32 workspace of at least
    attn_workspace_bytes(B, H, hd, ctx)."""
    if q.dim() != 3 or kcache.dim() != 4:
        raise ValueError(f"q / kcache: shapes {tuple(q.shape)} / {tuple(kcache.shape)}, expected "
                         "[B, H, hd] / [B, KVH, ctx, hd]")
    B, H, hd = q.shape
    KVH, ctx = kcache.shape[1], kcache.shape[2]
    _want_shape(B, H, KVH, hd, ctx)
    _want(q, "q", (B, H, hd))
    _want(kcache, "kcache", (B, KVH, ctx, hd))
    _want(vcache, "vcache", (B, KVH, ctx, hd))
    _want_pos(pos)
    _want(out, "out", (B, H * hd))
    if ws.dim() != 1:
        raise ValueError(f"ws: shape {tuple(ws.shape)}, expected one dimension")
    _want(ws, "ws", ws.shape, torch.float32)
    lib = _lib()
    need = lib.vgpu_attn_decode_workspace(B, H, hd, ctx)
    if ws.numel() * 4 < need:
        raise ValueError(f"ws: {ws.numel() * 4} bytes, needs {need}")
    _check(lib.vgpu_attn_decode(_p(q), _p(kcache), _p(vcache), _p(pos), _p(out), _p(ws), ws.numel() * 4, B, H, KVH,
                                hd, ctx, float(scale), _stream()), "vgpu_attn_decode")


def swiglu(gu: torch.Tensor, y: torch.Tensor) -> None:
    """y [B, ffn] = silu(g) * u from gu [B, 2 ffn] = [g | u]."""
    if gu.dim() != 2 or gu.shape[1] % 16 or gu.shape[1] < 16 or gu.shape[0] < 1:
        raise ValueError(f"gu: shape {tuple(gu.shape)}, expected [B, 2 ffn] with ffn % 8 == 0")
    B, ffn = gu.shape[0], gu.shape[1] // 2
    _want(gu, "gu", (B, 2 * ffn))
    _want(y, "y", (B, ffn))
    _check(_lib().vgpu_swiglu(_p(gu), _p(y), B, ffn, _stream()), "vgpu_swiglu")


def gemv(x: torch.Tensor, w: torch.Tensor, y: torch.Tensor) -> None:
    """y [B, N] = x [B, K] w[N, K]^T, no bias, on skinny.hip's forward kernel
    (B in 1-4 or 8, N % 4 == 0, K % 8 == 0): one pass over w."""
    if x.dim() != 2 or w.dim() != 2:
        raise ValueError(f"x / w: shapes {tuple(x.shape)} / {tuple(w.shape)}, expected [B, K] / [N, K]")
    B, K = x.shape
    N = w.shape[0]
    if B not in BATCHES or N % 4 or K % 8 or N < 4 or K < 8:
        raise ValueError(f"gemv: B {B}, N {N}, K {K} (needs B in {BATCHES}, N % 4 == 0, K % 8 == 0)")
    _want(x, "x", (B, K))
    _want(w, "w", (N, K))
    _want(y, "y", (B, N))
    _check(_lib().vgpu_skinny_fwd(_p(x), _p(w), None, _p(y), B, N, K, 0, _stream()), "vgpu_skinny_fwd")


def check_llama(model, tokens: torch.Tensor, kv_caches, at, *, prefill: bool, fp8: bool) -> None:
    """Everything decode_native and prefill_native of Llama and LlamaFp8 need
    of their arguments and weights.  prefill: `at` is `start`, a host int, and
    tokens are [B, S]; otherwise `at` is `pos`, a 1-element int64 tensor, and
    tokens are [B, 1].  fp8: the weights are LlamaFp8's buffers, typed by
    suffix; otherwise bf16 parameters.  Reasons come in one order: shapes,
    then layout and dtype of caches, weights and `at`, devices last."""
    from vgpu.ops import fp8 as Q, prefill as P  # both import this module
    cfg = model.cfg
    if prefill and (tokens.dim() != 2 or tokens.shape[1] < 1):
        raise ValueError(f"tokens: shape {tuple(tokens.shape)}, expected [B, S] with S >= 1")
    if not prefill and (tokens.dim() != 2 or tokens.shape[1] != 1):
        raise ValueError(f"tokens: shape {tuple(tokens.shape)}, expected [B, 1]")
    B, S = tokens.shape
    hd = cfg.dim // cfg.heads
    if len(kv_caches) != cfg.layers:
        raise ValueError(f"kv_caches: {len(kv_caches)} layers, expected {cfg.layers}")
    if cfg.layers and kv_caches[0][0].dim() != 4:
        raise ValueError(f"kv cache: shape {tuple(kv_caches[0][0].shape)}, expected [B, KVH, ctx, hd]")
    if prefill:
        ctx = kv_caches[0][0].shape[2] if cfg.layers else P._want_start(at) + S
        widths = {"dim": cfg.dim, "ffn": cfg.ffn, "qkv width": (cfg.heads + 2 * cfg.kv_heads) * hd, "vocab": cfg.vocab}
        for name, v in widths.items():
            if v < 64 or v % 64:
                raise ValueError(f"prefill shape not supported: {name} {v} not a multiple of 64")
        P._want_shape(B, S, P._want_start(at), cfg.heads, cfg.kv_heads, hd, ctx)
        if at + S > cfg.max_seq:
            raise ValueError(f"start {at} + {S} tokens > max_seq {cfg.max_seq} of the rope tables")
        for K, N in ((cfg.dim, widths["qkv width"]), (cfg.dim, 2 * cfg.ffn), (cfg.ffn, cfg.dim)):
            why = P.gemm_reason(B * S, K, N)
            if why:
                raise ValueError(f"prefill shape not supported: {why}")
    else:
        ctx = kv_caches[0][0].shape[2] if cfg.layers else 1
        _want_shape(B, cfg.heads, cfg.kv_heads, hd, ctx)
    if fp8:
        Q.check_llama_fp8_config(cfg)
    elif not prefill and (cfg.dim % 8 or cfg.ffn % 8 or cfg.vocab % 4):
        raise ValueError(f"decode shape not supported: dim {cfg.dim} / ffn {cfg.ffn} not multiples of 8, or vocab "
                         f"{cfg.vocab} not a multiple of 4")
    for i, (kc, vc) in enumerate(kv_caches):
        _want(kc, f"k cache of layer {i}", (B, cfg.kv_heads, ctx, hd), device=False)
        _want(vc, f"v cache of layer {i}", (B, cfg.kv_heads, ctx, hd), device=False)
    if fp8:
        weights = Q._check_buffers(model)
    else:
        weights = list(model.named_parameters())
        for name, p_ in weights:
            if not p_.is_contiguous():
                raise ValueError(f"{name}: not contiguous")
            if p_.dtype != BF16:
                raise ValueError(f"{name}: dtype {p_.dtype}, expected {BF16}")
    if prefill:
        if tokens.dtype != torch.int64:
            raise ValueError(f"tokens: dtype {tokens.dtype}, expected {torch.int64}")
    else:
        _want(at, "pos", (1,), torch.int64, device=False)
    on = [("tokens", tokens)] + ([] if prefill else [("pos", at)])
    on += [(f"kv cache of layer {i}", t) for i, kv in enumerate(kv_caches) for t in kv] + weights
    for name, t in on:
        if not t.is_cuda:
            raise ValueError(f"{name}: on {t.device}, expected a GPU tensor")
