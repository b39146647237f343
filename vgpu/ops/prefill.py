"""A Llama prompt on the native kernels: RoPE + KV-cache write for S tokens and
causal grouped-query flash attention over the cache (native/kernels/
prefill.hip), and the projections as bf16 MFMA GEMMs on the 1x1 path of
conv_gemm.hip.  The row kernels a prompt shares with a decode step
(add_rmsnorm, swiglu, and the GEMV of the head) are vgpu.ops.decode's.

`start`, the number of tokens already in the cache, is a host int: grids and
key ranges depend on it, so these launches are not replayed from a graph at
other positions.  Arguments are checked here, before the library is loaded; a
tensor the kernels cannot take raises ValueError naming the reason (never a
fall-back to eager)."""
from __future__ import annotations

import ctypes

import torch

from vgpu.native import load_kernels
from vgpu.ops.decode import BF16, HEAD_DIMS, MAX_GROUP, _p, _stream, _want

MAX_GRID = 65535       # B and H are grid dimensions
MAX_CTX = 1 << 30
INT32_MAX = 2 ** 31 - 1
_THREADS = 256
_BOUND = False


def _lib():
    global _BOUND
    lib = load_kernels()
    if not _BOUND:
        vp, ci, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_float
        lib.vgpu_prefill_supported.argtypes = [ci] * 7
        lib.vgpu_prefill_supported.restype = ci
        lib.vgpu_rope_kv_write_seq.argtypes = [vp] * 6 + [ci] * 8 + [vp]
        lib.vgpu_rope_kv_write_seq.restype = ci
        lib.vgpu_attn_prefill.argtypes = [vp] * 4 + [ci] * 7 + [cf, vp]
        lib.vgpu_attn_prefill.restype = ci
        lib.vgpu_conv2d_nhwc_ws.argtypes = [vp] * 7 + [ci] * 9 + [vp, ctypes.c_int64, vp]
        lib.vgpu_conv2d_nhwc_ws.restype = ci
        lib.vgpu_conv2d_workspace.argtypes = [ci] * 9
        lib.vgpu_conv2d_workspace.restype = ctypes.c_int64
        _BOUND = True
    return lib


def _check(rc, what):
    if rc == -1:
        raise ValueError(f"{what}: the library refused the arguments")
    if rc != 0:
        raise RuntimeError(f"{what}: error {rc}")


# ---- argument checks (no library, no device needed) -------------------------------------

def shape_reason(B: int, S: int, start: int, H: int, KVH: int, hd: int, ctx: int) -> str | None:
    """Why vgpu_prefill_supported refuses this shape (None: it takes it)."""
    if B < 1:
        return f"batch {B} < 1"
    if S < 1:
        return f"{S} prompt tokens (at least 1)"
    if start < 0:
        return f"start {start} < 0"
    if ctx < 1:
        return f"context {ctx} < 1"
    if start + S > ctx:
        return f"start {start} + {S} tokens > context {ctx}"
    if hd not in HEAD_DIMS:
        return f"head_dim {hd} not in {HEAD_DIMS}"
    if H < 1 or KVH < 1 or H % KVH:
        return f"heads {H} not a multiple of kv_heads {KVH}"
    if H // KVH > MAX_GROUP:
        return f"{H // KVH} query heads per kv head (at most {MAX_GROUP})"
    if B > MAX_GRID or H > MAX_GRID:
        return f"batch {B} or heads {H} > {MAX_GRID}"
    if ctx > MAX_CTX:
        return f"context {ctx} > {MAX_CTX}"
    if B * S * (H + 2 * KVH) * (hd // 16) > INT32_MAX - _THREADS:
        return f"{B} x {S} tokens of {H + 2 * KVH} heads: more 16-column items than a 32-bit index holds"
    return None


def _want_shape(B, S, start, H, KVH, hd, ctx) -> None:
    why = shape_reason(B, S, start, H, KVH, hd, ctx)
    if why:
        raise ValueError(f"prefill shape not supported: {why}")


def _want_all(*specs) -> None:
    """_want for each (tensor, name, shape[, dtype]); the device of any of them
    is looked at only when everything else about all of them is in order."""
    for t, name, shape, *dtype in specs:
        _want(t, name, shape, *dtype, device=False)
    for t, name, *_ in specs:
        if not t.is_cuda:
            raise ValueError(f"{name}: on {t.device}, expected a GPU tensor")


def _want_start(start) -> int:
    if isinstance(start, bool) or not isinstance(start, int):
        raise ValueError(f"start: {type(start).__name__}, expected a host int")
    return start


# ---- the kernels -----------------------------------------------------------------------

def rope_kv_write_seq(qkv: torch.Tensor, cos: torch.Tensor, sin: torch.Tensor, start: int, q_out: torch.Tensor,
                      kcache: torch.Tensor, vcache: torch.Tensor) -> None:
    """qkv [B S, (H + 2 KVH) hd] (row b S + s) -> rotated q into q_out
    [B, S, H, hd], rotated k and raw v into rows start .. start + S - 1 of the
    [B, KVH, ctx, hd] caches.  cos / sin are rope_tables' [max_seq, hd / 2] fp32."""
    if q_out.dim() != 4 or kcache.dim() != 4:
        raise ValueError(f"q_out / kcache: shapes {tuple(q_out.shape)} / {tuple(kcache.shape)}, expected "
                         "[B, S, H, hd] / [B, KVH, ctx, hd]")
    B, S, H, hd = q_out.shape
    KVH, ctx = kcache.shape[1], kcache.shape[2]
    _want_shape(B, S, _want_start(start), H, KVH, hd, ctx)
    if cos.dim() != 2 or cos.shape[0] < 1:
        raise ValueError(f"cos: shape {tuple(cos.shape)}, expected [max_seq, {hd // 2}]")
    max_seq = cos.shape[0]
    if start + S > max_seq:
        raise ValueError(f"start {start} + {S} tokens > max_seq {max_seq} of the rope tables")
    _want_all((qkv, "qkv", (B * S, (H + 2 * KVH) * hd)), (cos, "cos", (max_seq, hd // 2), torch.float32),
              (sin, "sin", (max_seq, hd // 2), torch.float32), (q_out, "q_out", (B, S, H, hd)),
              (kcache, "kcache", (B, KVH, ctx, hd)), (vcache, "vcache", (B, KVH, ctx, hd)))
    _check(_lib().vgpu_rope_kv_write_seq(_p(qkv), _p(cos), _p(sin), _p(q_out), _p(kcache), _p(vcache), B, S, start, H,
                                         KVH, hd, ctx, max_seq, _stream()), "vgpu_rope_kv_write_seq")


def attn_prefill(q: torch.Tensor, kcache: torch.Tensor, vcache: torch.Tensor, start: int, out: torch.Tensor,
                 scale: float) -> None:
    """out [B, S, H hd]: row i of head h is softmax(q_i K^T scale) V over cache
    rows 0 .. start + i of kv head h // (H / KVH)."""
    if q.dim() != 4 or kcache.dim() != 4:
        raise ValueError(f"q / kcache: shapes {tuple(q.shape)} / {tuple(kcache.shape)}, expected "
                         "[B, S, H, hd] / [B, KVH, ctx, hd]")
    B, S, H, hd = q.shape
    KVH, ctx = kcache.shape[1], kcache.shape[2]
    _want_shape(B, S, _want_start(start), H, KVH, hd, ctx)
    scale = float(scale)
    if not 0.0 < scale < float("inf"):
        raise ValueError(f"scale: {scale}, expected a positive finite number")
    _want_all((q, "q", (B, S, H, hd)), (kcache, "kcache", (B, KVH, ctx, hd)), (vcache, "vcache", (B, KVH, ctx, hd)),
              (out, "out", (B, S, H * hd)))
    _check(_lib().vgpu_attn_prefill(_p(q), _p(kcache), _p(vcache), _p(out), B, S, start, H, KVH, hd, ctx, scale,
                                    _stream()), "vgpu_attn_prefill")


def gemm_reason(M: int, K: int, N: int) -> str | None:
    """Why gemm refuses [M, K] x [N, K]^T (None: it takes it)."""
    if M < 1 or K < 64 or N < 64 or K % 64 or N % 64:
        return f"M {M}, K {K}, N {N} (needs M >= 1 and K, N positive multiples of 64)"
    # conv_gemm.hip addresses x and y of one image through 32-bit byte offsets
    # and runs no slice of less than one image; this GEMM is one image of M rows.
    if M * max(K, N) * 2 > INT32_MAX:
        return f"M {M} x max(K, N) {max(K, N)} bf16 is 2 GiB or more: beyond the kernel's 32-bit offsets"
    return None


def gemm(x: torch.Tensor, w: torch.Tensor, y: torch.Tensor) -> None:
    """y [M, N] = x [M, K] w[N, K]^T, no bias: the bf16 MFMA 1x1 convolution of
    conv_gemm.hip over one image of M x 1 pixels (w is nn.Linear's layout),
    split-K through the workspace the library asks for when M x N is small."""
    if x.dim() != 2 or w.dim() != 2:
        raise ValueError(f"x / w: shapes {tuple(x.shape)} / {tuple(w.shape)}, expected [M, K] / [N, K]")
    M, K = x.shape
    N = w.shape[0]
    why = gemm_reason(M, K, N)
    if why:
        raise ValueError(f"gemm: {why}")
    _want_all((x, "x", (M, K)), (w, "w", (N, K)), (y, "y", (M, N)))
    lib = _lib()
    need = lib.vgpu_conv2d_workspace(1, M, 1, K, N, 1, 1, 0, 0)
    if need < 0:
        raise ValueError(f"gemm: M {M}, K {K}, N {N}: the library refused the shape")
    ws = torch.empty(need // 4, dtype=torch.float32, device=x.device) if need > 0 else None
    _check(lib.vgpu_conv2d_nhwc_ws(_p(x), _p(w), _p(y), None, None, None, None, 1, M, 1, K, N, 1, 1, 0, 0, _p(ws),
                                   need, _stream()), "vgpu_conv2d_nhwc_ws")

