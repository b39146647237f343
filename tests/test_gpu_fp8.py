"""native/kernels/gemv_fp8.hip and LlamaFp8 on the GPU.

References: G1 and G4 compare with torch's own reading of the 256 e4m3fn
codes, bit for bit; G2 with int64 sums (test_fp8_cpu.py C3 shows them exact in
fp32 in any order, C4 that they catch a wrong decode, byte order, scale row or
batch row); G3 with fp64; G6 and G8's decode steps with fp64 decode_static of
the dequantised model on the CPU; G7 and G8's prompt with the same values run
another way, bit for bit.  No reference or bound comes from the kernels.

Every buffer a kernel writes through a direct library call is followed by 16
guard rows of 0xFF bytes that must stay intact."""
import ctypes

import pytest
import torch

import _decode_ref as R
import _fp8_ref as Q
from vgpu.models.llama import LlamaFp8
from vgpu.ops.decode import BATCHES

pytestmark = pytest.mark.gpu

BF, F64 = R.BF, R.F64
Guarded = Q.Guarded


@pytest.fixture(scope="module")
def lib(gpu_build):
    from vgpu.ops import fp8 as F
    return F._lib()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gemv(lib, x, codes, scale):
    """vgpu_gemv_fp8 on CPU tensors -> y [B, N] on the CPU; the output's guard rows checked."""
    B, K = x.shape
    N = codes.shape[0]
    y = Guarded(B, N)
    xg, cg, sg = x.cuda(), codes.cuda(), scale.cuda()  # held until the kernel has run
    rc = lib.vgpu_gemv_fp8(_ptr(xg), _ptr(cg), _ptr(sg), y.ptr, B, N, K, _stream())
    assert rc == 0, (B, N, K)
    torch.cuda.synchronize()
    assert y.intact(), (B, N, K)
    return y.t.cpu()


# ---- G1 decode table ---------------------------------------------------------------------

@pytest.mark.parametrize("K", [32, 4096 + 16])
@pytest.mark.parametrize("B", [1, 3])
def test_g1_decode_table(lib, B, K):
    """Row n holds code n at column k0 and 0x00 elsewhere; a one-hot x reads the
    kernel's decoding of every code at every byte position of two adjacent
    16-byte loads.  At B = 3: row 1 is one-hot at another column (zeros), row
    2 holds 2 at k0 (twice the table)."""
    table = Q.TABLE.float()
    for k0 in range(32):
        codes = torch.zeros(256, K, dtype=torch.uint8)
        codes[:, k0] = torch.arange(256, dtype=torch.uint8)
        x = torch.zeros(B, K)
        x[0, k0] = 1
        want = [table]
        if B == 3:
            x[1, (k0 + 7) % 32] = 1
            x[2, k0] = 2
            want += [torch.zeros(256), 2 * table]
        y = _gemv(lib, x.to(BF), codes, torch.ones(256)).float()
        for b in range(B):
            assert bool(torch.isnan(y[b][~Q.FINITE]).all()), (k0, b)
            assert torch.equal(y[b][Q.FINITE], want[b][Q.FINITE]), (k0, b)


# ---- G2 exact integers -------------------------------------------------------------------

def test_g2_edges_are_the_kernels(lib):
    """The K edges of the exact cases are named from the kernel's K loop."""
    from vgpu.ops import fp8 as F
    assert (Q.K_LANE, Q.K_WAVE, Q.K_BLOCK) == (F.K_LANE, F.K_WAVE, F.K_BLOCK)
    assert lib.vgpu_gemv_fp8_trip() == Q.TRIP and Q.TRIP % Q.K_BLOCK == 0
    for k in (Q.K_LANE, Q.K_WAVE, Q.K_BLOCK, Q.TRIP):
        assert {max(k - 16, 16), k, k + 16} <= set(Q.K_EDGES)


@pytest.mark.parametrize("N,K", Q.EXACT_NK)
def test_g2_exact_integers(lib, N, K):
    for B in BATCHES:
        x, codes, scale = Q.exact_case(B, N, K)
        want = Q.exact_expected(x, codes, scale)
        first = _gemv(lib, x, codes, scale)
        assert torch.equal(first, want), (B, (first.float() - want.float()).abs().max().item())
        assert torch.equal(_gemv(lib, x, codes, scale), first), B


# ---- G3 real values ----------------------------------------------------------------------

@pytest.mark.parametrize("N,K", [(512, 512), (64, 14336)])
@pytest.mark.parametrize("B", [1, 3, 8])
def test_g3_real_values(lib, B, N, K):
    """|y - ref| <= 2^-8 |ref| + K 2^-23 sum_k |x_k w_nk|: one bf16 rounding with
    this project's margin, and the worst case of an fp32 sum of K terms in any
    order.  Row 5 carries a scale that is no power of two."""
    from vgpu.ops import fp8 as F
    g = torch.Generator().manual_seed(B + N + K)
    x = torch.randn(B, K, generator=g).to(BF)
    codes, scale = F.quantize((torch.randn(N, K, generator=g) * 0.02).to(BF))
    scale[5] = 0.75 * 2.0 ** -10
    w = Q.TABLE[codes.long()] * scale.to(F64)[:, None]
    ref = x.to(F64) @ w.T
    mag = x.to(F64).abs() @ w.abs().T
    y = _gemv(lib, x, codes, scale).to(F64)
    err = (y - ref).abs()
    lim = 2.0 ** -8 * ref.abs() + K * 2.0 ** -23 * mag
    print(f"B {B} N {N} K {K}: max err {err.max().item():.3e}, max err / bound {(err / lim).max().item():.3f}")
    assert bool(torch.isfinite(y).all()) and bool((err <= lim).all())


# ---- G4 dequant --------------------------------------------------------------------------

def _dequant(lib, codes, scale):
    N, K = codes.shape
    out = Guarded(N, K)
    cg, sg = codes.cuda(), scale.cuda()  # held until the kernel has run
    assert lib.vgpu_dequant_fp8(_ptr(cg), _ptr(sg), out.ptr, N, K, _stream()) == 0
    torch.cuda.synchronize()
    assert out.intact()
    return out.t.cpu()


def test_g4_dequant(lib):
    from vgpu.ops import fp8 as F
    # code (r + k) % 256 in row r, column k: all 256 codes at each of 32 column positions, under three scales
    codes = ((torch.arange(768)[:, None] + torch.arange(32)[None, :]) % 256).to(torch.uint8)
    scale = torch.tensor([2.0 ** -12, 1.0, 2.0 ** 5]).repeat_interleave(256)
    got = _dequant(lib, codes, scale)
    want = (Q.TABLE[codes.long()] * scale.to(F64)[:, None])
    finite = Q.FINITE[codes.long()]
    assert torch.equal(want[finite].to(BF).to(F64), want[finite]), "scale * table is a bf16 value"
    assert torch.equal(got.to(F64)[finite], want[finite])
    assert bool(torch.isnan(got.float()[~finite]).all())
    g = torch.Generator().manual_seed(4)
    codes, scale = F.quantize((torch.randn(128, 4096, generator=g) * 0.02).to(BF))
    assert torch.equal(_dequant(lib, codes, scale), F.dequantize_ref(codes, scale, BF))


# ---- G5 the shape rule -------------------------------------------------------------------

def test_g5_supported_agrees_with_gemv_reason(lib):
    from vgpu.ops.fp8 import gemv_reason
    for B in range(10):
        for N in (0, 2, 4, 6, 8):
            for K in (0, 8, 16, 24, 32):
                assert bool(lib.vgpu_gemv_fp8_supported(B, N, K)) == (gemv_reason(B, N, K) is None), (B, N, K)
    x = torch.zeros(8, 32, dtype=BF, device="cuda")
    c, s, y = torch.zeros(8, 32, dtype=torch.uint8, device="cuda"), torch.ones(8, device="cuda"), torch.zeros_like(x)
    for B, N, K in ((5, 8, 32), (1, 6, 32), (1, 8, 24), (0, 8, 32), (1, 0, 32), (1, 8, 0)):
        assert lib.vgpu_gemv_fp8(_ptr(x), _ptr(c), _ptr(s), _ptr(y), B, N, K, _stream()) == -1, (B, N, K)
    assert lib.vgpu_dequant_fp8(_ptr(c), _ptr(s), _ptr(y), 8, 24, _stream()) == -1
    assert lib.vgpu_dequant_fp8(_ptr(c), _ptr(s), _ptr(y), 0, 32, _stream()) == -1


# ---- G6 decode end to end ----------------------------------------------------------------

@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("ci", [0, 1])
def test_g6_decode_native_end_to_end(gpu_build, ci, B):
    """e_native <= 2 e_eager, both the largest logit error over all 22 steps
    against fp64 decode_static of the dequantised model (so the quantisation
    error is in neither), and test_gpu_decode.py G5's cache requirement.
    Measured on an MI355X, e_eager / e_native: config 0 B 1 0.0219 / 0.0162,
    B 2 0.0139 / 0.0117; config 1 B 1 0.1038 / 0.0999, B 2 0.0216 / 0.0194
    (logits up to 2.5)."""
    ref = Q.decode_reference(ci, B)
    toks = R.tokens(ci, B)
    q = LlamaFp8.from_llama(R.model(ci), device="cuda")
    kv = R.new_cache(q, B, R.CTX, BF, "cuda")
    got = R.run_steps(q, q.decode_native, toks[:20], kv, R.STEPS[:20], "cuda")
    Q.cache_ok(kv, ref, torch.arange(20), "after 20 steps")
    got = torch.cat([got, R.run_steps(q, q.decode_native, toks[20:], kv, R.STEPS[20:], "cuda")])
    Q.cache_ok(kv, ref, torch.tensor(R.STEPS), "after all steps")
    assert got.shape == ref["f64"].shape and torch.isfinite(got).all()
    e_native = (got - ref["f64"]).abs().max().item()
    print(f"config {ci} B {B}: e_eager {ref['e_eager']:.4e} e_native {e_native:.4e}, "
          f"max |logit| {ref['f64'].abs().max().item():.3f}")
    assert e_native <= 2 * ref["e_eager"]


# ---- G7 graph replay ---------------------------------------------------------------------

def test_g7_graph_replay(gpu_build):
    ci, B = 0, 1
    toks = R.tokens(ci, B)[:20].cuda()
    q = LlamaFp8.from_llama(R.model(ci), device="cuda")
    kv_plain = R.new_cache(q, B, R.CTX, BF, "cuda")
    pos = torch.zeros(1, dtype=torch.long, device="cuda")
    want = []
    for p in range(20):
        pos.fill_(p)
        want.append(q.decode_native(toks[p], kv_plain, pos).clone())

    kv = R.new_cache(q, B, R.CTX, BF, "cuda")
    tok = toks[0].clone()
    pos.fill_(0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            q.decode_native(tok, kv, pos)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = q.decode_native(tok, kv, pos)
    torch.cuda.synchronize()
    for k, v in kv:  # the warm-up and the capture wrote row 0; start from the plain run's first state
        k.fill_(R.FILL)
        v.fill_(R.FILL)
    for p in range(20):
        pos.fill_(p)
        tok.copy_(toks[p])
        graph.replay()
        assert torch.equal(out, want[p]), p
    for (k, v), (kp, vp) in zip(kv, kv_plain):
        assert torch.equal(k, kp) and torch.equal(v, vp)


# ---- G8 prefill --------------------------------------------------------------------------

def _same_caches(a, b):
    return all(torch.equal(ka, kb) and torch.equal(va, vb) for (ka, va), (kb, vb) in zip(a, b))


@pytest.mark.parametrize("S", [1, Q.PROMPT])
@pytest.mark.parametrize("B", [1, 2])
def test_g8_prefill(gpu_build, B, S):
    """prefill_native of the fp8 model against prefill_native of its dequantised
    bf16 model: logits and every cache row equal, from start = 0 and in two
    chunks; then three decode_native steps from that cache within G6's bound.
    Measured on an MI355X, e_eager / e_native of those steps: B 1 0.0112 /
    0.0118, B 2 0.0117 / 0.0130."""
    ci = 0
    q = LlamaFp8.from_llama(R.model(ci), device="cuda")
    d = q.dequantized()
    assert next(d.parameters()).is_cuda
    prompt, dec = Q.prompt_tokens(ci, B)
    prompt = prompt[:, :S].cuda()
    kv_q, kv_d = R.new_cache(q, B, R.CTX, BF, "cuda"), R.new_cache(q, B, R.CTX, BF, "cuda")
    got, want = q.prefill_native(prompt, kv_q, 0), d.prefill_native(prompt, kv_d, 0)
    assert torch.isfinite(got.float()).all() and torch.equal(got, want)
    assert _same_caches(kv_q, kv_d)
    assert all(bool((k[:, :, S:] == R.FILL).all()) and bool((k[:, :, :S] != R.FILL).any()) for k, _ in kv_q)
    if S < sum(Q.CHUNKS):
        return
    kv_q2, kv_d2 = R.new_cache(q, B, R.CTX, BF, "cuda"), R.new_cache(q, B, R.CTX, BF, "cuda")
    c0 = Q.CHUNKS[0]
    for model, kv in ((q, kv_q2), (d, kv_d2)):
        model.prefill_native(prompt[:, :c0], kv, 0)
    got2, want2 = q.prefill_native(prompt[:, c0:], kv_q2, c0), d.prefill_native(prompt[:, c0:], kv_d2, c0)
    assert torch.equal(got2, want2) and _same_caches(kv_q2, kv_d2)
    ref = Q.decode_after_prompt_reference(ci, B)
    steps = R.run_steps(q, q.decode_native, dec, kv_q, Q.DECODE_POS, "cuda")
    e_native = (steps - ref["f64"]).abs().max().item()
    print(f"B {B}: decode after the prompt: e_eager {ref['e_eager']:.4e} e_native {e_native:.4e}")
    assert torch.isfinite(steps).all() and e_native <= 2 * ref["e_eager"]
