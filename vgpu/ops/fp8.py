"""Projection weights as OCP fp8 (e4m3fn) codes with one fp32 scale per output
row (native/kernels/gemv_fp8.hip): the quantiser, the decode GEMV over the
codes, and their expansion to bf16 for the prefill GEMM.

The format: a weight W [N, K] is `codes` [N, K] uint8 (the bit patterns of
torch.float8_e4m3fn: bias 7, 0x7F / 0xFF NaN, no infinities; not MI300X's
fnuz) and `scale` [N] fp32; element (n, k) is scale[n] * e4m3(codes[n, k]).
The kernels take any positive finite scale.  `quantize` emits powers of two,
so that scale * e4m3(code), at most 4 significant bits, is exact in bf16: the
bf16 model `dequantize_ref` builds holds exactly what the fp8 model computes
with, and the two can be compared bit for bit.

Arguments are checked here, before the library is loaded; a tensor the
kernels cannot take raises ValueError naming the reason (never a fall-back to
eager)."""
from __future__ import annotations

import ctypes

import torch

from vgpu.native import load_kernels
from vgpu.ops import prefill as P
from vgpu.ops.decode import BATCHES, BF16, _p, _stream
from vgpu.ops.prefill import _want_all

K_MULTIPLE = 16        # codes per 16-byte load
# the K loop of gemv_fp8_kernel, in columns: a lane's chunk, a wave's 64 chunks, the block's 256
K_LANE, K_WAVE, K_BLOCK = 16, 64 * 16, 256 * 16
_BOUND = False


def _lib():
    global _BOUND
    lib = load_kernels()
    if not _BOUND:
        vp, ci = ctypes.c_void_p, ctypes.c_int
        lib.vgpu_gemv_fp8_supported.argtypes = [ci] * 3
        lib.vgpu_gemv_fp8_supported.restype = ci
        lib.vgpu_gemv_fp8_trip.argtypes = []
        lib.vgpu_gemv_fp8_trip.restype = ci
        lib.vgpu_gemv_fp8.argtypes = [vp] * 4 + [ci] * 3 + [vp]
        lib.vgpu_gemv_fp8.restype = ci
        lib.vgpu_dequant_fp8.argtypes = [vp] * 3 + [ci] * 2 + [vp]
        lib.vgpu_dequant_fp8.restype = ci
        _BOUND = True
    return lib


# ---- the format, in pure torch (CPU or GPU) ---------------------------------------------

def e4m3_table(device=None) -> torch.Tensor:
    """The fp32 value of each of the 256 codes (0x7F and 0xFF: NaN), from the bit fields."""
    c = torch.arange(256, device=device)
    e, m = (c >> 3) & 15, (c & 7).float()
    mag = torch.where(e == 0, m * 2.0 ** -9, (8 + m) * torch.exp2((e - 10).float()))
    mag = torch.where((c & 0x7F) == 0x7F, torch.full_like(mag, float("nan")), mag)
    return torch.where(c >= 128, -mag, mag)


def _row_scales(amax: torch.Tensor) -> torch.Tensor:
    """Per row, the smallest power of two s (a normal fp32) with amax / s <= 448; 1 for a zero row."""
    f, e = torch.frexp(amax)                       # amax = f 2^e, f in [0.5, 1); 448 = 0.875 2^9
    t = torch.where(f <= 0.875, e - 9, e - 8).clamp(min=-126)
    return torch.where(amax > 0, torch.exp2(t.float()), torch.ones_like(amax))


def _round_e4m3(q: torch.Tensor) -> torch.Tensor:
    """fp32 q with |q| <= 448 -> uint8 codes, round to nearest, ties to the even
    code, subnormals included.  Integer and exact power-of-two arithmetic only,
    so the same path serves a build without the fp8 cast on the device."""
    a = q.abs()
    _, e = torch.frexp(a)
    E = torch.where(a < 2.0 ** -6, torch.full_like(e, -6), e - 1)  # the binade; -6 holds zero and the subnormals too
    r = torch.round(a * torch.exp2((3 - E).float()))  # a in units of 2^(E - 3): exact, ties to even; 0 .. 16
    code = ((E + 7) << 3) + r.to(torch.int32) - 8  # r = 16 carries into the next exponent by itself
    code = code + (torch.signbit(q).to(torch.int32) << 7)
    return code.to(torch.uint8)


def quantize(w: torch.Tensor, rows_at_once: int = 4096) -> tuple[torch.Tensor, torch.Tensor]:
    """w [N, K] (floating) -> (codes [N, K] uint8, scale [N] fp32) on w's device.
    scale[n] is the smallest power of two with max|w[n]| / scale[n] <= 448 (1
    for an all-zero row), codes are w / scale rounded to nearest-even into
    e4m3fn; 0x7F and 0xFF are never emitted.  Works through `rows_at_once`
    rows at a time, so the fp32 temporaries stay a fraction of the weight."""
    if w.dim() != 2:
        raise ValueError(f"w: shape {tuple(w.shape)}, expected [N, K]")
    if not w.dtype.is_floating_point:
        raise ValueError(f"w: dtype {w.dtype}, expected a floating dtype")
    N, K = w.shape
    codes = torch.empty((N, K), dtype=torch.uint8, device=w.device)
    scale = torch.empty((N,), dtype=torch.float32, device=w.device)
    for n0 in range(0, N, rows_at_once):
        wf = w[n0:n0 + rows_at_once].detach().float()
        if not bool(torch.isfinite(wf).all()):
            raise ValueError(f"w: rows {n0} .. {n0 + wf.shape[0] - 1} hold a value that is not finite")
        s = _row_scales(wf.abs().amax(dim=1)) if K else torch.ones(wf.shape[0], device=w.device)
        scale[n0:n0 + rows_at_once] = s
        codes[n0:n0 + rows_at_once] = _round_e4m3(wf / s[:, None])
    return codes, scale


def dequantize_ref(codes: torch.Tensor, scale: torch.Tensor, dtype=BF16) -> torch.Tensor:
    """scale[n] * e4m3(codes[n, k]) as `dtype`: the product in fp32 (in fp64 for
    dtype float64), then one rounding.  Exact for power-of-two scales."""
    if codes.dim() != 2 or codes.dtype != torch.uint8:
        raise ValueError(f"codes: shape {tuple(codes.shape)} dtype {codes.dtype}, expected [N, K] {torch.uint8}")
    if tuple(scale.shape) != (codes.shape[0],):
        raise ValueError(f"scale: shape {tuple(scale.shape)}, expected {(codes.shape[0],)}")
    wide = torch.float64 if dtype == torch.float64 else torch.float32
    table = e4m3_table(codes.device).to(wide)
    return (table[codes.to(torch.int32)] * scale.to(wide)[:, None]).to(dtype)


# ---- argument checks (no library, no device needed) -------------------------------------

def gemv_reason(B: int, N: int, K: int) -> str | None:
    """Why vgpu_gemv_fp8_supported refuses this shape (None: it takes it)."""
    if B not in BATCHES:
        return f"batch {B} not in {BATCHES}"
    if N < 4 or N % 4:
        return f"N {N} not a positive multiple of 4"
    if K < K_MULTIPLE or K % K_MULTIPLE:
        return f"K {K} not a positive multiple of {K_MULTIPLE}"
    return None


# ---- the kernels -----------------------------------------------------------------------

def gemv_fp8(x: torch.Tensor, codes: torch.Tensor, scale: torch.Tensor, y: torch.Tensor) -> None:
    """y [B, N] = bf16(scale[n] * sum_k x[b, k] e4m3(codes[n, k])): x, y bf16,
    fp32 accumulation, no bias (B in 1-4 or 8, N % 4 == 0, K % 16 == 0)."""
    if x.dim() != 2 or codes.dim() != 2:
        raise ValueError(f"x / codes: shapes {tuple(x.shape)} / {tuple(codes.shape)}, expected [B, K] / [N, K]")
    B, K = x.shape
    N = codes.shape[0]
    why = gemv_reason(B, N, K)
    if why:
        raise ValueError(f"gemv_fp8: {why}")
    _want_all((x, "x", (B, K)), (codes, "codes", (N, K), torch.uint8), (scale, "scale", (N,), torch.float32),
              (y, "y", (B, N)))
    P._check(_lib().vgpu_gemv_fp8(_p(x), _p(codes), _p(scale), _p(y), B, N, K, _stream()), "vgpu_gemv_fp8")


def dequant(codes: torch.Tensor, scale: torch.Tensor, out: torch.Tensor) -> None:
    """out [N, K] bf16 = bf16(scale[n] * e4m3(codes[n, k])), K % 16 == 0."""
    if codes.dim() != 2:
        raise ValueError(f"codes: shape {tuple(codes.shape)}, expected [N, K]")
    N, K = codes.shape
    if N < 1 or K < K_MULTIPLE or K % K_MULTIPLE:
        raise ValueError(f"dequant: N {N}, K {K} (needs N >= 1 and K a positive multiple of {K_MULTIPLE})")
    _want_all((codes, "codes", (N, K), torch.uint8), (scale, "scale", (N,), torch.float32), (out, "out", (N, K)))
    P._check(_lib().vgpu_dequant_fp8(_p(codes), _p(scale), _p(out), N, K, _stream()), "vgpu_dequant_fp8")


# ---- LlamaFp8's arguments ----------------------------------------------------------------

def check_llama_fp8_config(cfg) -> None:
    """What the fp8 GEMV asks of a Llama's widths (from_llama, and decode.check_llama for both steps)."""
    hd = cfg.dim // cfg.heads
    widths = {"dim": cfg.dim, "ffn": cfg.ffn, "attention width": cfg.heads * hd}
    for name, v in widths.items():
        if v < K_MULTIPLE or v % K_MULTIPLE:
            raise ValueError(f"fp8 shape not supported: {name} {v} not a multiple of {K_MULTIPLE}")
    for name, v in (("qkv width", (cfg.heads + 2 * cfg.kv_heads) * hd), ("vocab", cfg.vocab)):
        if v < 4 or v % 4:
            raise ValueError(f"fp8 shape not supported: {name} {v} not a multiple of 4")


def _check_buffers(model) -> list:
    """Every buffer of a LlamaFp8 contiguous and of its dtype; returns them for the device check."""
    named = list(model.named_buffers())
    for name, t in named:
        if not t.is_contiguous():
            raise ValueError(f"{name}: not contiguous")
    for name, t in named:
        want = torch.uint8 if name.endswith("codes") else torch.float32 if name.endswith("scale") else BF16
        if t.dtype != want:
            raise ValueError(f"{name}: dtype {t.dtype}, expected {want}")
    return named

