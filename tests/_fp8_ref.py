"""Shared by test_fp8_cpu.py and test_gpu_fp8.py: the e4m3fn table as torch
decodes it, the exact-integer GEMV cases with their expected outputs (and the
same outputs under five deliberate mistakes), guarded buffers, and the CPU
references of the end-to-end fp8 decode and prefill tests.  Nothing here comes
from the kernels under test."""
import copy
import ctypes
import functools

import torch

import _decode_ref as R
from vgpu.ops.decode import BATCHES

BF, F64 = R.BF, R.F64

# the 256 codes as torch's own float8_e4m3fn reads them (0x7F, 0xFF: NaN)
TABLE = torch.arange(256, dtype=torch.uint8).view(torch.float8_e4m3fn).to(F64)
FINITE = torch.isfinite(TABLE)
# the same bits read as MI300X's e4m3fnuz: bias 8, 0x80 NaN, no negative zero
_c = torch.arange(256)
_e, _m = (_c >> 3) & 15, (_c & 7).to(F64)
_mag = torch.where(_e == 0, _m * 2.0 ** -10, (8 + _m) * torch.exp2((_e - 11).to(F64)))
TABLE_FNUZ = torch.where(_c >= 128, -_mag, _mag)
TABLE_FNUZ[128] = float("nan")


def code_of(v: torch.Tensor) -> torch.Tensor:
    """The e4m3fn code of each value of v (values the table holds; +0 for zero)."""
    vals = TABLE.clone()
    vals[128] = float("nan")  # -0: never chosen
    uniq, inverse = torch.unique(v.to(F64), return_inverse=True)
    hit = uniq[:, None] == vals
    assert bool(hit.any(-1).all())
    return hit.to(torch.uint8).argmax(-1).to(torch.uint8)[inverse]


class Guarded:
    """rows x width elements for a kernel to write, then 16 sentinel rows of 0xFF bytes."""

    def __init__(self, rows, width, dtype=BF, fill=None):
        n = rows * width * torch.empty((), dtype=dtype).element_size()
        self.raw = torch.full((n // rows * (rows + 16),), 0xFF, dtype=torch.uint8, device="cuda")
        self.t = self.raw[:n].view(dtype).view(rows, width)
        self.tail = self.raw[n:]
        if fill is not None:
            self.t.copy_(fill)

    @property
    def ptr(self):
        return ctypes.c_void_p(self.t.data_ptr())

    def intact(self):
        return bool((self.tail == 0xFF).all())


# ---- G2 / C3 / C4: exact integers ---------------------------------------------------------
# The K loop of gemv_fp8_kernel, in columns: a lane takes a 16-column chunk, a
# wave 64 chunks, the block's four waves 256, and one trip of the loop TRIP
# columns (vgpu.ops.fp8 names the first three; the library reports the trip:
# one chunk per lane in the shipped kernel, so a trip is the block's stride;
# 2 TRIP stays among the edges as the start of a third trip).
K_LANE, K_WAVE, K_BLOCK = 16, 1024, 4096
TRIP = 4096
K_EDGES = sorted({16} | {k + d for k in (K_LANE, K_WAVE, K_BLOCK, TRIP, 2 * TRIP) for d in (-16, 0, 16) if k + d >= 16})
EXACT_NK = [(n, k) for n in (4, 8, 4 * 37) for k in K_EDGES] + [(8, 14336)]  # Llama-3-8B's K: 4096 (an edge) and 14336
EXACT_CASES = [(b, n, k) for n, k in EXACT_NK for b in BATCHES]


@functools.lru_cache(maxsize=None)
def exact_case(B, N, K):
    """x [B, K] bf16 integers in [-4, 4], codes [N, K] of integers in [-8, 8],
    scale [N]: powers of two from 2^-3 to 2^3, neighbours differing."""
    g = torch.Generator().manual_seed(1000 * B + 7 * N + K)
    x = torch.randint(-4, 5, (B, K), generator=g)
    w = torch.randint(-8, 9, (N, K), generator=g)
    scale = torch.exp2(((torch.arange(N) * 3) % 7 - 3).float())
    return x.to(BF), code_of(w), scale


def exact_sums(x, codes, table=TABLE):
    """sum_k x w exactly (fp64 holds every partial sum of these cases), and sum_k |x w|."""
    w = table[codes.long()]
    x64 = x.to(F64)
    return x64 @ w.T, x64.abs() @ w.abs().T


def exact_expected(x, codes, scale, table=TABLE):
    """bf16(fp32(sum) * scale): the sum is an integer below 2^24 and the scale a
    power of two, so the fp32 product is exact and bf16 is the only rounding."""
    s, _ = exact_sums(x, codes, table)
    return (s.to(torch.float32) * scale[None, :]).to(BF)


def mistakes(x, codes, scale):
    """name -> the output a kernel with that one mistake would give."""
    N, K = codes.shape
    out = {
        "fnuz": exact_expected(x, codes, scale, TABLE_FNUZ),
        "bytes of each word reversed": exact_expected(x, codes.view(N, K // 4, 4).flip(-1).reshape(N, K), scale),
        "16-bit halves swapped": exact_expected(x, codes.view(N, K // 4, 2, 2).flip(2).reshape(N, K), scale),
        "scale of row n + 1": exact_expected(x, codes, scale.roll(-1)),
        "scale of row n - 1": exact_expected(x, codes, scale.roll(1)),
    }
    if x.shape[0] > 1:
        out["batch rows swapped"] = exact_expected(x.flip(0), codes, scale)
    return out


# ---- G6 / G8: the fp8 model's values, run on the CPU ----------------------------------------

@functools.lru_cache(maxsize=None)
def fp8_model(ci):
    from vgpu.models.llama import LlamaFp8
    return LlamaFp8.from_llama(R.model(ci))


@functools.lru_cache(maxsize=None)
def dequantized(ci):
    """bf16 Llama on the CPU holding exactly what fp8_model(ci) represents."""
    return fp8_model(ci).dequantized()


def dequantized_as(ci, dtype, device="cpu"):
    return copy.deepcopy(dequantized(ci)).to(dtype).to(device)


@functools.lru_cache(maxsize=None)
def decode_reference(ci, b):
    """_decode_ref.reference for the dequantised model: fp64 and bf16
    decode_static on the CPU over R.STEPS.  Quantisation error is in neither."""
    toks = R.tokens(ci, b)
    res = {}
    for name, dtype in (("f64", F64), ("bf16", BF)):
        m = dequantized_as(ci, dtype)
        kv = R.new_cache(m, b, R.CTX, dtype)
        res[name] = R.run_steps(m, m.decode_static, toks, kv, R.STEPS)
        res[name + "_kv"] = kv
    res["e_eager"] = (res["bf16"] - res["f64"]).abs().max().item()
    return res


PROMPT = 70
CHUNKS = (40, 30)
DECODE_POS = [70, 71, 72]


@functools.lru_cache(maxsize=None)
def prompt_tokens(ci, b):
    """([b, 70] prompt, [3, b, 1] tokens of the decode steps after it)."""
    g = torch.Generator().manual_seed(1900 + 10 * ci + b)
    vocab = R.CONFIGS[ci].vocab
    return torch.randint(0, vocab, (b, PROMPT), generator=g), torch.randint(0, vocab, (3, b, 1), generator=g)


@functools.lru_cache(maxsize=None)
def decode_after_prompt_reference(ci, b):
    """forward(prompt) then three decode_static steps of the dequantised model
    on the CPU, fp64 and bf16: the steps' logits and the eager run's error."""
    prompt, dec = prompt_tokens(ci, b)
    res = {}
    for name, dtype in (("f64", F64), ("bf16", BF)):
        m = dequantized_as(ci, dtype)
        kv = R.new_cache(m, b, R.CTX, dtype)
        with torch.no_grad():
            m(prompt, kv, 0)
        res[name] = R.run_steps(m, m.decode_static, dec, kv, DECODE_POS)
    res["e_eager"] = (res["bf16"] - res["f64"]).abs().max().item()
    return res


def cache_ok(kv, ref, written, what):
    """test_gpu_decode.py's cache requirement: rows in `written` against the
    fp64 run's (layer 0 within one bf16 ulp at the largest magnitude those rows
    hold, deeper layers within twice the eager bf16 run's own error), every
    other row still 64.0."""
    ctx = kv[0][0].shape[2]
    rest = torch.ones(ctx, dtype=torch.bool)
    rest[written] = False
    for i, (pair, ref_pair, eager_pair) in enumerate(zip(kv, ref["f64_kv"], ref["bf16_kv"])):
        for name, t, r64, eager in zip("kv", pair, ref_pair, eager_pair):
            t = t.cpu()
            assert bool((t[:, :, rest] == R.FILL).all()), (what, i, name)
            ref_w = r64[:, :, written]
            ulp = 2.0 ** -7 * ref_w.abs().max().item()
            e_eager = (eager[:, :, written].to(F64) - ref_w).abs().max().item()
            err = (t[:, :, written].to(F64) - ref_w).abs().max().item()
            print(f"{what} layer {i} {name}: max err {err:.3e}, eager's {e_eager:.3e}, one ulp {ulp:.3e}")
            assert err <= (ulp if i == 0 else 2 * e_eager), (what, i, name)
