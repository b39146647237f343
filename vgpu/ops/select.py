"""Choosing the next token on the device (native/kernels/select.hip): greedy
argmax and temperature / top-k / top-p sampling over bf16 logits [B, V], each
fused with the bookkeeping that closes a decode loop: the token goes to
`out[:, step]` and to `next_tok` (the buffer the next embedding reads), then
`step` and `pos` advance by one, all on the device, so decode + select captures
into one graph that replays with no host work in between.

Ordering of logits: by value with +0 == -0, NaN below -inf, ties to the lowest
index (a row of all NaN selects index 0).  `top_p` acts inside the top-k set; a
nucleus over the whole vocabulary is not provided.

Arguments are checked here, before the library is loaded; anything the kernels
cannot take raises ValueError naming the reason (never a fall-back to eager)."""
from __future__ import annotations

import ctypes
import math

import torch

from vgpu.native import load_kernels
from vgpu.ops.decode import BATCHES, BF16, _check, _p, _stream, _want

MAX_TOP_K = 64
MAX_VOCAB = 1 << 30
_BOUND = False


def _lib():
    global _BOUND
    lib = load_kernels()
    if not _BOUND:
        vp, ci, i64, cf = ctypes.c_void_p, ctypes.c_int, ctypes.c_int64, ctypes.c_float
        lib.vgpu_select_supported.argtypes = [ci] * 3
        lib.vgpu_select_supported.restype = ci
        lib.vgpu_select_chunk.argtypes = [ci]
        lib.vgpu_select_chunk.restype = ci
        lib.vgpu_select_workspace.argtypes = [ci, ci]
        lib.vgpu_select_workspace.restype = i64
        lib.vgpu_select_greedy.argtypes = [vp, vp, i64, ci, ci, vp, vp, vp, vp, ci, ci, vp]
        lib.vgpu_select_greedy.restype = ci
        lib.vgpu_select_sample.argtypes = [vp, vp, i64, ci, ci, cf, ci, cf, vp, vp, vp, vp, vp, ci, ci, vp]
        lib.vgpu_select_sample.restype = ci
        _BOUND = True
    return lib


# ---- argument checks (no library, no device needed) -------------------------------------

def shape_reason(B: int, V: int, top_k: int = 1) -> str | None:
    """Why vgpu_select_supported refuses this shape (None: it takes it)."""
    if B not in BATCHES:
        return f"batch {B} not in {BATCHES}"
    if V < 8 or V % 8 or V > MAX_VOCAB:
        return f"vocab {V} not a multiple of 8 in 8 .. {MAX_VOCAB}"
    if not 1 <= top_k <= MAX_TOP_K:
        return f"top_k {top_k} not in 1 .. {MAX_TOP_K}"
    return None


def params_reason(temperature: float, top_k: int, top_p: float) -> str | None:
    """Why these sampling parameters are refused (None: they are taken)."""
    if not (math.isfinite(temperature) and temperature > 0):
        return f"temperature {temperature} not a finite number above 0"
    if not isinstance(top_k, int) or isinstance(top_k, bool) or not 1 <= top_k <= MAX_TOP_K:
        return f"top_k {top_k} not an integer in 1 .. {MAX_TOP_K}"
    if not 0 < top_p <= 1:
        return f"top_p {top_p} not in (0, 1]"
    return None


def _want_common(logits, ws, step, pos, next_tok, out, eos, top_k, u=None):
    if logits.dim() != 2:
        raise ValueError(f"logits: shape {tuple(logits.shape)}, expected [B, V]")
    B, V = logits.shape
    why = shape_reason(B, V, top_k)
    if why:
        raise ValueError(f"select shape not supported: {why}")
    if out.dim() != 2 or out.shape[0] != B or out.shape[1] < 1:
        raise ValueError(f"out: shape {tuple(out.shape)}, expected [{B}, T] with T >= 1")
    T = out.shape[1]
    if not isinstance(eos, int) or isinstance(eos, bool) or not -1 <= eos < V:
        raise ValueError(f"eos: {eos!r}, expected -1 (none) or a token id below {V}")
    if ws.dim() != 1:
        raise ValueError(f"ws: shape {tuple(ws.shape)}, expected one dimension")
    # per tensor shape, layout, dtype; the device of all of them last, so the
    # reason named is the first that holds on any machine
    named = [("logits", logits, (B, V), BF16), ("step", step, (1,), torch.int64), ("pos", pos, (1,), torch.int64),
             ("next_tok", next_tok, (B, 1), torch.int64), ("out", out, (B, T), torch.int64),
             ("ws", ws, ws.shape, torch.int32)]
    if u is not None:
        named.append(("u", u, (T, B), torch.float32))
    for name, t, shape, dtype in named:
        _want(t, name, shape, dtype, device=False)
    for name, t, _, _ in named:
        if not t.is_cuda:
            raise ValueError(f"{name}: on {t.device}, expected a GPU tensor")
    return B, V, T


def _want_ws(lib, ws, B, V):
    need = lib.vgpu_select_workspace(B, V)
    if ws.numel() * 4 < need:
        raise ValueError(f"ws: {ws.numel() * 4} bytes, needs {need}")


# ---- the kernels -----------------------------------------------------------------------

def chunk(V: int) -> int:
    """Logits per workgroup of the partial launches (the tests aim at its edges)."""
    why = shape_reason(1, V)
    if why:
        raise ValueError(f"select shape not supported: {why}")
    return int(_lib().vgpu_select_chunk(V))


def workspace_bytes(B: int, V: int) -> int:
    why = shape_reason(B, V)
    if why:
        raise ValueError(f"select shape not supported: {why}")
    return int(_lib().vgpu_select_workspace(B, V))


def greedy(logits: torch.Tensor, ws: torch.Tensor, step: torch.Tensor, pos: torch.Tensor, next_tok: torch.Tensor,
           out: torch.Tensor, eos: int = -1) -> None:
    """With s = step[0]: out[b, s] = next_tok[b, 0] = the first index of row b
    of logits [B, V] (bf16) in the ordering of the module docstring, or `eos`
    once out[b, s - 1] == eos (eos -1: never); then step += 1 and pos += 1.  s
    outside [0, T) writes nothing.  step, pos [1], next_tok [B, 1], out [B, T]:
    int64 on the GPU; ws: int32 workspace of at least workspace_bytes(B, V)."""
    B, V, T = _want_common(logits, ws, step, pos, next_tok, out, eos, 1)
    lib = _lib()
    _want_ws(lib, ws, B, V)
    _check(lib.vgpu_select_greedy(_p(logits), _p(ws), ws.numel() * 4, B, V, _p(step), _p(pos), _p(next_tok), _p(out),
                                  T, eos, _stream()), "vgpu_select_greedy")


def sample(logits: torch.Tensor, ws: torch.Tensor, step: torch.Tensor, pos: torch.Tensor, next_tok: torch.Tensor,
           out: torch.Tensor, u: torch.Tensor, temperature: float, top_k: int, top_p: float = 1.0,
           eos: int = -1) -> None:
    """greedy() with a draw in place of the argmax.  Candidates c_0 .. c_{k-1}
    are the first k = top_k (at most MAX_TOP_K) indices of the row in the
    ordering; a non-finite l[c_0] gives c_0.  Otherwise, in fp32, w_j =
    exp((l[c_j] - l[c_0]) / temperature) (0 for a NaN candidate), W_k their
    sum, the nucleus the smallest m >= 1 with sum_{j<m} w_j >= top_p W_k, and
    the token c_j for the smallest j < m with sum_{i<=j} w_i > u[s, b] W_m
    (c_{m-1} if rounding leaves none).  u: [T, B] fp32 uniforms in [0, 1), row
    s read.  top_p acts inside the top-k set only."""
    why = params_reason(temperature, top_k, top_p)
    if why:
        raise ValueError(f"select parameters not supported: {why}")
    B, V, T = _want_common(logits, ws, step, pos, next_tok, out, eos, top_k, u)
    lib = _lib()
    _want_ws(lib, ws, B, V)
    _check(lib.vgpu_select_sample(_p(logits), _p(ws), ws.numel() * 4, B, V, float(temperature), top_k, float(top_p),
                                  _p(u), _p(step), _p(pos), _p(next_tok), _p(out), T, eos, _stream()),
           "vgpu_select_sample")
