"""native/kernels/prefill.hip, the GEMM of vgpu.ops.prefill and
Llama.prefill_native against fp64 on the CPU.

References: P1-P3 compute the kernel's own formula in fp64 from the bf16
inputs; P4 uses `forward` (and, after the prompt, decode_static) of the fp64
model on the CPU.  No bound is taken from the kernels; P2's is derived in
test_p2_attn_prefill, and test_prefill_cpu.py shows on the CPU that it tells
the right arithmetic from a mask off by one and from a wrong head mapping.

Every buffer a kernel writes through a direct call is allocated with 16
further rows of 0xFF bytes, and those rows must be untouched afterwards.
Cache rows a kernel has no business with hold 64.0: finite, and 20 or more
standard deviations from any k or v.

Which test fails for which mistake (argued from prefill.hip):
  * mask off by one: P2's bound by 6 x or more, the v[0] identity at row 0,
    and prefix invariance at every row it samples.
  * GQA head mapping wrong: P2 at (H, KVH) = (4, 2), (8, 2), (8, 1).
  * a key tile's tail, or a cache row >= start + S, read: P2 through the 64.0
    fill (and nothing beyond ctx exists in the ctx == start + S cases).
  * query rows >= S of a tail tile stored: the sentinel rows behind `out`.
  * NaN out of an all-masked tile row: S = 65 / 129 (rows whose last tile is
    masked whole for them while other rows of the wave still have keys there).
  * K swizzle or V transpose wrong: every P2 case (hd = 64 and 128 stage differently).
  * cache row index, stride or rotation wrong: P1.
  * chunked prompt not equal to the one-shot one, or a cache decode cannot
    read: P4.
"""
import ctypes

import pytest
import torch

import _decode_ref as R
import _prefill_ref as PR
from vgpu.models.llama import LlamaConfig, rope_tables

pytestmark = pytest.mark.gpu

BF, F64 = R.BF, R.F64
CTX = R.CTX


@pytest.fixture(scope="module")
def P(gpu_build):
    from vgpu.ops import prefill as mod
    mod._lib()
    return mod


@pytest.fixture(scope="module")
def lib(P):
    return P._lib()


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


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _bound_ok(got, ref, rel, extra, what):
    """|got - ref| <= rel |ref| + extra, elementwise (fp64 on the CPU)."""
    err = (got.to(F64) - ref).abs()
    lim = rel * ref.abs() + extra
    worst = (err - lim).max().item()
    print(f"{what}: max err {err.max().item():.3e}, max (err - bound) {worst:.3e}")
    assert torch.isfinite(got.to(F64)).all(), what
    assert worst <= 0.0, what


# ---- P1 rope_kv_write_seq --------------------------------------------------------------

def _rope64(x, cos, sin):
    """x [..., hd] bf16 -> fp64 rotation (first half pairs with second half) and its bound's |x1| + |x2|."""
    x1, x2 = x.to(F64).chunk(2, dim=-1)
    c, s = cos.to(F64), sin.to(F64)
    mag = x1.abs() + x2.abs()
    return torch.cat([x1 * c - x2 * s, x1 * s + x2 * c], dim=-1), torch.cat([mag, mag], dim=-1)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("H,KVH", PR.HEADS)
@pytest.mark.parametrize("B", [1, 3])
def test_p1_rope_kv_write_seq(lib, B, H, KVH, hd):
    max_seq = 256
    cos, sin = rope_tables(LlamaConfig(dim=hd, heads=1, max_seq=max_seq))
    cg, sg = cos.cuda(), sin.cuda()
    fill = torch.full((B * KVH * CTX, hd), R.FILL, dtype=BF)
    heads = H + 2 * KVH

    def run(qkv, S, start):
        kc, vc = Guarded(B * KVH * CTX, hd, fill=fill), Guarded(B * KVH * CTX, hd, fill=fill)
        qg = Guarded(B * S * H, hd)
        rc = lib.vgpu_rope_kv_write_seq(_ptr(qkv.cuda()), _ptr(cg), _ptr(sg), qg.ptr, kc.ptr, vc.ptr, B, S, start, H,
                                        KVH, hd, CTX, max_seq, _stream())
        torch.cuda.synchronize()
        assert kc.intact() and vc.intact() and qg.intact(), (S, start)
        return rc, qg.t.cpu().view(B, S, H, hd), kc.t.cpu().view(B, KVH, CTX, hd), vc.t.cpu().view(B, KVH, CTX, hd)

    for S, start in [(1, 0), (5, 0), (67, 0), (5, 59), (1, 159), (96, 64)]:  # the last two end exactly at ctx
        qkv = torch.randn(B * S, heads * hd, generator=_gen(S + start + hd + H)).to(BF)
        rc, q_got, k_got, v_got = run(qkv, S, start)
        assert rc == 0, (S, start)
        q, k, v = qkv.view(B, S, heads, hd).split([H, KVH, KVH], dim=2)
        c, s = cos[start:start + S, None], sin[start:start + S, None]  # [S, 1, hd / 2] against [B, S, heads, hd / 2]
        written = slice(start, start + S)
        for name, got, src in (("q", q_got, q), ("k", k_got[:, :, written].transpose(1, 2), k)):
            ref, mag = _rope64(src, c, s)
            _bound_ok(got, ref, 2.0 ** -8, 2.0 ** -20 * mag, f"{name} at S {S} start {start}")
        assert torch.equal(v_got[:, :, written].transpose(1, 2), v), (S, start)
        rest = torch.ones(CTX, dtype=torch.bool)
        rest[written] = False
        assert bool((k_got[:, :, rest] == R.FILL).all()) and bool((v_got[:, :, rest] == R.FILL).all()), (S, start)

    for S, start in [(1, CTX), (5, CTX - 4), (CTX + 1, 0)]:  # start + S = ctx + 1: refused, nothing written
        qkv = torch.randn(B * S, heads * hd, generator=_gen(S)).to(BF)
        rc, _, k_got, v_got = run(qkv, S, start)
        assert rc == -1, (S, start)
        assert bool((k_got == R.FILL).all()) and bool((v_got == R.FILL).all()), (S, start)
    # a table shorter than start + S is refused as well
    qkv = torch.randn(B * 5, heads * hd, generator=_gen(5)).to(BF)
    kc = Guarded(B * KVH * CTX, hd, fill=fill)
    assert lib.vgpu_rope_kv_write_seq(_ptr(qkv.cuda()), _ptr(cg), _ptr(sg), Guarded(B * 5 * H, hd).ptr, kc.ptr, kc.ptr,
                                      B, 5, 59, H, KVH, hd, CTX, 63, _stream()) == -1
    torch.cuda.synchronize()
    assert bool((kc.t == R.FILL).all())


# ---- P2 attn_prefill -------------------------------------------------------------------

def _attn_gpu(lib, case, q, kg, vg, scale):
    B, H, KVH, hd, S, start, ctx = case
    out = Guarded(B * S, H * hd)
    rc = lib.vgpu_attn_prefill(_ptr(q), _ptr(kg), _ptr(vg), out.ptr, B, S, start, H, KVH, hd, ctx, scale, _stream())
    assert rc == 0, case
    torch.cuda.synchronize()
    assert out.intact(), case
    return out.t.cpu().view(B, S, H, hd)


@pytest.mark.parametrize("case", PR.P2_CASES, ids=PR.case_id)
def test_p2_attn_prefill(lib, case):
    """|got - ref| <= 2^-7 A elementwise, A = softmax · |V| in fp64.

    A rounding to bf16 is off by up to 2^-8 of the value.  P rounded into the
    PV product: at most 2^-8 A in the numerator, and that only if every key's
    rounding error had the sign of its v; over many keys they largely cancel.
    l is summed from the unrounded P in fp32 and adds nothing of that size.
    The output rounding: 2^-8 |ref| <= 2^-8 A.  Together at most 2^-7 A, the
    bound, with fp32 accumulation over n <= 2^9 keys (under 2^-14 A) covered by
    that cancellation.  Measured on an MI355X, the kernel uses at most 0.81 of
    the bound over these 138 cases, as the emulation of its arithmetic does on
    the CPU; there a mask off by one is 6 x or more outside the bound and a
    wrong head mapping 77 x or more (test_prefill_cpu.py)."""
    B, H, KVH, hd, S, start, ctx = case
    q, k, v, scale = PR.p2_inputs(case)
    ref, A = PR.attn64(q, k, v, start, scale)
    qg, kg, vg = q.cuda(), k.cuda(), v.cuda()
    got = _attn_gpu(lib, case, qg, kg, vg, scale)
    again = _attn_gpu(lib, case, qg, kg, vg, scale)
    assert torch.isfinite(got.float()).all()
    assert torch.equal(got, again)
    used = PR.excess(got, ref, A)
    print(f"{PR.case_id(case)}: {used:.3f} of the bound")
    assert used <= 1.0
    if start == 0:  # row 0 sees key 0 alone: its value row, bit for bit
        assert torch.equal(got[:, 0], v[:, :, 0].repeat_interleave(H // KVH, dim=1))


@pytest.mark.parametrize("case", PR.PREFIX_CASES, ids=PR.case_id)
def test_p2_prefix_invariance(lib, case):
    """Rows 0 .. i do not change by a bit when cache rows > start + i are
    overwritten: a masked key contributes an exact zero and does not enter the maximum."""
    B, H, KVH, hd, S, start, ctx = case
    q, k, v, scale = PR.p2_inputs(case)
    qg = q.cuda()
    first = _attn_gpu(lib, case, qg, k.cuda(), v.cuda(), scale)
    for i in (0, 31, 32, 63, 64, S - 2):
        k2, v2 = k.clone(), v.clone()
        k2[:, :, start + i + 1:] = R.FILL
        v2[:, :, start + i + 1:] = R.FILL
        got = _attn_gpu(lib, case, qg, k2.cuda(), v2.cuda(), scale)
        assert torch.equal(got[:, :i + 1], first[:, :i + 1]), i


# ---- P3 gemm ---------------------------------------------------------------------------

@pytest.mark.parametrize("M,K,N", [(1, 64, 64), (77, 512, 1024), (130, 1024, 512), (300, 256, 2048)])
def test_p3_gemm(P, M, K, N):
    g = _gen(M + K + N)
    x = torch.randn(M, K, generator=g).to(BF)
    w = (torch.randn(N, K, generator=g) * K ** -0.5).to(BF)
    y = Guarded(M, N)
    P.gemm(x.cuda(), w.cuda(), y.t)
    torch.cuda.synchronize()
    ref = x.to(F64) @ w.to(F64).t()
    _bound_ok(y.t.cpu(), ref, 2.0 ** -8, K * 2.0 ** -23 * (x.to(F64).abs() @ w.to(F64).abs().t()), "y")
    assert y.intact()


def test_p3_gemm_refuses(P):
    def z(*shape):
        return torch.zeros(shape, dtype=BF, device="cuda")
    with pytest.raises(ValueError, match="K 72"):
        P.gemm(z(4, 72), z(64, 72), z(4, 64))
    with pytest.raises(ValueError, match="N 96"):
        P.gemm(z(4, 64), z(96, 64), z(4, 96))


# ---- P4 end to end ---------------------------------------------------------------------

def _cache_ok(kv, ref, what):
    """Rows 0 .. 36 against the fp64 run's, every other row still 64.0 (the rule
    of test_gpu_decode's _cache_ok).  Layer 0: within one bf16 ulp at the
    largest magnitude the reference holds in those rows, since its input is
    the embedding row, the same bits in every run.  Deeper layers: within
    twice the eager bf16 run's own error against fp64 on the same rows."""
    n = PR.PROMPT
    for i, (pair, ref_pair, eager_pair) in enumerate(zip(kv, ref["f64_kv"], ref["bf16_kv"])):
        for name, t, r64, eager in zip("kv", pair, ref_pair, eager_pair):
            t = t.cpu()
            assert bool((t[:, :, n:] == R.FILL).all()), (what, i, name)
            ref_w = r64[:, :, :n]
            ulp = 2.0 ** -7 * ref_w.abs().max().item()
            e_eager = (eager[:, :, :n].to(F64) - ref_w).abs().max().item()
            err = (t[:, :, :n].to(F64) - ref_w).abs().max().item()
            print(f"{what} layer {i} {name}: max err {err:.3e}, eager's {e_eager:.3e}, one ulp {ulp:.3e}")
            assert err <= (ulp if i == 0 else 2 * e_eager), (what, i, name)


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("ci", [0, 1])
def test_p4_prefill_native_end_to_end(P, ci, B):
    """e_native <= 2 e_eager, both the largest logit error against the fp64
    `forward` on the CPU; then three decode_native steps on the cache the
    prefill wrote, and the same prompt in two chunks, under the same rule.
    Measured on an MI355X, e_eager / e_native (ratios 0.89-1.09): config 0 B 1
    0.0097 / 0.0101, B 2 0.0099 / 0.0098; config 1 B 1 0.0158 / 0.0172, B 2
    0.0174 / 0.0154 (logits up to 2.4); chunked equal to one shot to the digits
    printed; the decode steps 0.0106-0.0199 / 0.0120-0.0200 (ratios 0.95-1.13)."""
    ref = PR.p4_reference(ci, B)
    prompt, dec = PR.p4_tokens(ci, B)
    m = R.model_as(ci, BF, "cuda")
    tg = prompt.cuda()

    kv = R.new_cache(m, B, CTX, BF, "cuda")
    got = m.prefill_native(tg, kv, 0)
    assert got.shape == (B, 1, m.cfg.vocab)
    got = got[:, 0].to(F64).cpu()
    assert torch.isfinite(got).all()
    _cache_ok(kv, ref, "one shot")
    e_native = (got - ref["f64"]).abs().max().item()
    print(f"config {ci} B {B}: e_eager {ref['e_eager']:.4e} e_native {e_native:.4e}, "
          f"max |logit| {ref['f64'].abs().max().item():.3f}")
    assert e_native <= 2 * ref["e_eager"]

    # hand-over to decode: positions 37, 38, 39 on the cache the prefill wrote
    got_dec = R.run_steps(m, m.decode_native, dec, kv, PR.DECODE_POS, "cuda")
    assert torch.isfinite(got_dec).all()
    e_dec = (got_dec - ref["f64_dec"]).abs().max().item()
    print(f"config {ci} B {B} decode after prefill: e_eager {ref['e_eager_dec']:.4e} e_native {e_dec:.4e}")
    assert e_dec <= 2 * ref["e_eager_dec"]

    # the prompt in two chunks, on fresh caches
    kv2 = R.new_cache(m, B, CTX, BF, "cuda")
    m.prefill_native(tg[:, :20].contiguous(), kv2, 0)
    got2 = m.prefill_native(tg[:, 20:].contiguous(), kv2, 20)[:, 0].to(F64).cpu()
    assert torch.isfinite(got2).all()
    _cache_ok(kv2, ref, "chunked")
    e_chunked = (got2 - ref["f64"]).abs().max().item()
    print(f"config {ci} B {B} chunked: e_native {e_chunked:.4e}")
    assert e_chunked <= 2 * ref["e_eager"]


# ---- P5 refusals -----------------------------------------------------------------------

def test_p5_shapes_refused(lib):
    """vgpu_prefill_supported's rules, and the Python check that mirrors them."""
    from vgpu.ops.prefill import shape_reason
    seen = set()
    for B in (0, 1, 9):
        for S in (0, 1):
            for start in (-1, 0):
                for over in (0, 1):  # start + S = ctx, ctx + 1
                    for hd in (32, 64, 96, 128, 256):
                        for H, KVH in ((32, 8), (32, 5), (32, 2), (8, 8)):
                            case = (B, S, start, H, KVH, hd, start + S - over)
                            ok = bool(lib.vgpu_prefill_supported(*case))
                            assert ok == (shape_reason(*case) is None), case
                            seen.add(ok)
    assert seen == {True, False}
    for case in ((1, 2048, 0, 32, 8, 128, 8192), (9, 37, 100, 8, 1, 64, 137), (70000, 1, 0, 8, 8, 64, 8),
                 (1, 1, 0, 70000, 70000, 64, 8), (8, 2 ** 20, 0, 32, 8, 128, 2 ** 20), (1, 1, 0, 8, 8, 64, 2 ** 30 + 1)):
        assert bool(lib.vgpu_prefill_supported(*case)) == (shape_reason(*case) is None), case
