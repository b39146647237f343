"""The fp8 weight format on the CPU: the quantiser's properties (C1), every
refusal of the fp8 entry points before any library is loaded (C2), and the
soundness (C3) and sharpness (C4) of the exact-integer cases the GPU test of
the GEMV runs."""
import pytest
import torch

import _decode_ref as R
import _fp8_ref as Q
from vgpu.models.llama import Llama, LlamaConfig, LlamaFp8
from vgpu.ops import fp8 as F

BF, F64 = R.BF, R.F64


# ---- C1 ----------------------------------------------------------------------------------

def _adversarial_rows():
    """[rows, 64] bf16, each row one of the issue's hard cases (see the names)."""
    K = 64
    rows, names = [], []

    def add(name, head):
        r = torch.zeros(K, dtype=F64)
        r[:len(head)] = torch.tensor(head, dtype=F64)
        rows.append(r)
        names.append(name)

    add("all zero", [])
    add("one element", [0.0, -0.3125])
    for e in (-9, 0, 5):
        s = 2.0 ** e
        add(f"max exactly 448 * 2^{e}", [448 * s, -3 * s, 17 * s, 0.375 * s])
        add(f"max just above 448 * 2^{e}", [-450 * s, 446 * s, 3 * s, 200 * s])  # 450: the next bf16 after 448
        # deep in the row's subnormal range: ties at 2^-10 (to code 0) and 3 * 2^-10 (to code 2), their neighbours,
        # the smallest normal 2^-6 and the value half a step under it
        add(f"subnormals under 448 * 2^{e}",
            [448 * s] + [v * s for v in (2.0 ** -10, 1.0078125 * 2.0 ** -10, 0.99609375 * 2.0 ** -10, 3 * 2.0 ** -10,
                                         5 * 2.0 ** -10, 2.0 ** -9, 2.0 ** -7, 2.0 ** -6, 15 * 2.0 ** -10,
                                         7.5 * 2.0 ** -9, -2.0 ** -12, 2.0 ** -20, -7 * 2.0 ** -9)])
        add(f"max rounds down to 224 * 2^{e}", [228 * s, -100 * s, 2.0 ** -8 * s])
    w = torch.stack(rows).to(BF)
    assert torch.equal(w.to(F64), torch.stack(rows)), "every adversarial value is a bf16 value"
    return w, names


def _matrices():
    g = torch.Generator().manual_seed(11)
    yield "N(0, 0.02)", (torch.randn(24, 64, generator=g) * 0.02).to(BF)
    yield "rows of every magnitude", (torch.randn(24, 64, generator=g)
                                      * torch.exp2(torch.randint(-40, 40, (24, 1), generator=g).float())).to(BF)
    yield "heavy tails", (torch.randn(24, 64, generator=g) ** 5).to(BF)
    yield "adversarial", _adversarial_rows()[0]


@pytest.mark.parametrize("name,w", list(_matrices()), ids=[n for n, _ in _matrices()])
def test_c1_quantiser(name, w):
    codes, scale = F.quantize(w)
    assert codes.dtype == torch.uint8 and codes.shape == w.shape and scale.dtype == torch.float32
    w64, s64 = w.to(F64), scale.to(F64)
    amax = w64.abs().amax(1)
    # the smallest power of two with max / s <= 448; 1 for a zero row
    assert bool((torch.frexp(scale)[0] == 0.5).all()), "scales are powers of two"
    assert bool((amax / s64 <= 448).all())
    assert bool(((amax / (s64 / 2) > 448) | (amax == 0)).all())
    assert bool((scale[amax == 0] == 1).all())
    # never a NaN code
    assert not bool(((codes & 0x7F) == 0x7F).any())
    # half a unit of e4m3 in each range
    q = w64 / s64[:, None]
    val = Q.TABLE[codes.long()] * s64[:, None]
    err = (w64 - val).abs()
    normal = q.abs() >= 2.0 ** -6
    assert bool((err[normal] <= 2.0 ** -4 * w64.abs()[normal]).all())
    assert bool((err <= s64[:, None] * 2.0 ** -10)[~normal].all())
    # the nearest of the 254 finite values by exhaustive search, ties to the even code
    dist = (q[..., None] - Q.TABLE).abs()
    dist[..., ~Q.FINITE] = float("inf")
    near = dist == dist.amin(-1, keepdim=True)
    assert bool(near.gather(-1, codes.long()[..., None]).all()), "a code that is not the nearest value"
    tie = (near.sum(-1) == 2) & (q != 0)
    assert name != "adversarial" or int(tie.sum()) >= 6
    assert bool((codes[tie] % 2 == 0).all()), "a tie not rounded to the even code"
    assert torch.equal(codes[q == 0], (torch.signbit(w)[q == 0].to(torch.uint8) << 7))
    # bf16 holds the represented value exactly
    deq = F.dequantize_ref(codes, scale, BF)
    assert torch.equal(deq.to(F64), val)
    assert torch.equal(F.dequantize_ref(codes, scale, F64), val)
    # Quantising the represented values again.  They are a fixed point: the same
    # values come back, always.  The pair (codes, scale) comes back too, except
    # for a row whose largest element was rounded down to 224 s: 224 s is
    # 448 (s / 2), and "the smallest power of two with max / s <= 448" of the
    # rounded row is s / 2.  (The issue asks for the pair unconditionally; with
    # its own rule for the scale that cannot hold for such rows, about one row
    # in 28.  Here: the pair where it can hold, s / 2 where it cannot.)
    codes2, scale2 = F.quantize(deq)
    assert torch.equal(F.dequantize_ref(codes2, scale2, F64), val)
    halved = (val.abs().amax(1) / s64) == 224
    assert torch.equal(codes2[~halved], codes[~halved]) and torch.equal(scale2[~halved], scale[~halved])
    assert torch.equal(scale2[halved], scale[halved] / 2)
    assert name != "adversarial" or int(halved.sum()) >= 3


def test_c1_table_and_refused_inputs():
    """The table built from the bit fields is torch's, bit for bit; what quantize cannot take is refused."""
    t = F.e4m3_table()
    assert torch.equal(torch.isnan(t), ~Q.FINITE)
    assert torch.equal(t[Q.FINITE].to(F64), Q.TABLE[Q.FINITE])
    assert torch.equal(torch.signbit(t), torch.arange(256) >= 128)
    for bad, why in ((torch.zeros(4), "shape"), (torch.zeros(4, 16, dtype=torch.int32), "dtype"),
                     (torch.full((4, 16), float("inf")), "not finite"), (torch.full((4, 16), float("nan")), "not finite")):
        with pytest.raises(ValueError, match=why):
            F.quantize(bad)


# ---- C2 ----------------------------------------------------------------------------------

@pytest.fixture
def no_library(monkeypatch):
    from vgpu.ops import decode as D, prefill as P

    def no_load():
        raise AssertionError("the native library was loaded before the arguments were checked")
    for mod in (F, D, P):
        monkeypatch.setattr(mod, "load_kernels", no_load)


def test_c2_kernel_refusals(no_library):
    x, y = torch.zeros(2, 32, dtype=BF), torch.zeros(2, 8, dtype=BF)
    codes, scale = torch.zeros(8, 32, dtype=torch.uint8), torch.ones(8)
    out = torch.zeros(8, 32, dtype=BF)
    wide = torch.zeros(8, 64, dtype=torch.uint8)
    gemv_cases = [
        ((x[0], codes, scale, y), "expected \\[B, K\\] / \\[N, K\\]"),
        ((torch.zeros(5, 32, dtype=BF), codes, scale, torch.zeros(5, 8, dtype=BF)), "batch 5"),
        ((x, codes[:6], scale[:6], y[:, :6]), "N 6"),
        ((x[:, :24], codes[:, :24], scale, y), "K 24"),
        ((x, wide, scale, y), "codes: shape"),
        ((x, codes, scale[:4], y), "scale: shape"),
        ((x, codes, scale, y[:, :4]), "y: shape"),
        ((x, wide[:, ::2], scale, y), "codes: not contiguous"),
        ((x, codes.to(torch.int8), scale, y), "codes: dtype"),
        ((x.float(), codes, scale, y), "x: dtype"),
        ((x, codes, scale.double(), y), "scale: dtype"),
        ((x, codes, scale, y), "x: on cpu, expected a GPU tensor"),
    ]
    for args, why in gemv_cases:
        with pytest.raises(ValueError, match=why):
            F.gemv_fp8(*args)
    dequant_cases = [
        ((codes[0], scale, out), "expected \\[N, K\\]"),
        ((codes[:, :24], scale, out[:, :24]), "K 24"),
        ((codes, scale, out[:4]), "out: shape"),
        ((codes, scale[:4], out), "scale: shape"),
        ((wide[:, ::2], scale, out), "codes: not contiguous"),
        ((codes, scale, out.float()), "out: dtype"),
        ((codes.to(torch.int8), scale, out), "codes: dtype"),
        ((codes, scale, out), "codes: on cpu, expected a GPU tensor"),
    ]
    for args, why in dequant_cases:
        with pytest.raises(ValueError, match=why):
            F.dequant(*args)
    assert F.gemv_reason(1, 4, 16) is None and F.gemv_reason(8, 128256, 14336) is None
    for bad in ((0, 4, 16), (5, 4, 16), (1, 0, 16), (1, 6, 16), (1, 4, 0), (1, 4, 8), (1, 4, 24)):
        assert F.gemv_reason(*bad), bad


def test_c2_from_llama_refusals(no_library):
    with pytest.raises(ValueError, match="expected a Llama"):
        LlamaFp8.from_llama(torch.nn.Linear(16, 16))
    with pytest.raises(ValueError, match="dim 24 not a multiple of 16"):
        LlamaFp8.from_llama(Llama(LlamaConfig(vocab=64, dim=24, layers=1, heads=1, kv_heads=1, ffn=32, max_seq=8)))
    with pytest.raises(ValueError, match="ffn 40 not a multiple of 16"):
        LlamaFp8.from_llama(Llama(LlamaConfig(vocab=64, dim=32, layers=1, heads=1, kv_heads=1, ffn=40, max_seq=8)))
    with pytest.raises(ValueError, match="vocab 66 not a multiple of 4"):
        LlamaFp8.from_llama(Llama(LlamaConfig(vocab=66, dim=32, layers=1, heads=1, kv_heads=1, ffn=32, max_seq=8)))
    m = Llama(LlamaConfig(vocab=64, dim=32, layers=2, heads=1, kv_heads=1, ffn=32, max_seq=8))
    with torch.no_grad():
        m.layers[1].w2.weight[3, 5] = float("inf")
    with pytest.raises(ValueError, match="layers.1.w2: .*not finite"):
        LlamaFp8.from_llama(m)


def _fresh(ci=0):
    return LlamaFp8.from_llama(R.model(ci))


def test_c2_decode_native_refusals(no_library):
    q = _fresh()
    assert all(not b.is_cuda for b in q.buffers())
    pos = torch.zeros(1, dtype=torch.long)
    tok = R.tokens(0, 1)[0]

    def cache(b=1, dtype=BF):
        return R.new_cache(q, b, R.CTX, dtype)

    with pytest.raises(ValueError, match="tokens: on cpu, expected a GPU tensor"):
        q.decode_native(tok, cache(), pos)
    with pytest.raises(ValueError, match="expected \\[B, 1\\]"):
        q.decode_native(tok[0], cache(), pos)
    with pytest.raises(ValueError, match="1 layers, expected 2"):
        q.decode_native(tok, cache()[:1], pos)
    kv = [(k.transpose(1, 2).contiguous().transpose(1, 2), v) for k, v in cache()]
    with pytest.raises(ValueError, match="not contiguous"):
        q.decode_native(tok, kv, pos)
    with pytest.raises(ValueError, match="k cache of layer 0: dtype"):
        q.decode_native(tok, cache(dtype=torch.float32), pos)
    with pytest.raises(ValueError, match="batch 5"):
        q.decode_native(tok.expand(5, 1), cache(5), pos)
    with pytest.raises(ValueError, match="pos: dtype"):
        q.decode_native(tok, cache(), pos.int())
    tiny = LlamaFp8.from_llama(Llama(LlamaConfig.tiny()))
    with pytest.raises(ValueError, match="head_dim 32"):
        tiny.decode_native(tok, tiny.new_kv_cache(1, 64), pos)
    # the model's own buffers
    q.layers[1].wo.scale = q.layers[1].wo.scale.double()
    with pytest.raises(ValueError, match="layers.1.wo.scale: dtype"):
        q.decode_native(tok, cache(), pos)
    q = _fresh()
    q.head.codes = q.head.codes.to(torch.int8)
    with pytest.raises(ValueError, match="head.codes: dtype"):
        q.decode_native(tok, cache(), pos)
    q = _fresh()
    q.layers[0].norm2 = q.layers[0].norm2.float()
    with pytest.raises(ValueError, match="layers.0.norm2: dtype"):
        q.decode_native(tok, cache(), pos)
    q = _fresh()
    q.layers[0].w13.codes = q.layers[0].w13.codes.t().contiguous().t()
    with pytest.raises(ValueError, match="layers.0.w13.codes: not contiguous"):
        q.decode_native(tok, cache(), pos)
    q = _fresh()
    q.cfg = LlamaConfig(**{**vars(q.cfg), "ffn": 1032})
    with pytest.raises(ValueError, match="ffn 1032 not a multiple of 16"):
        q.decode_native(tok, cache(), pos)


def test_c2_prefill_native_refusals(no_library):
    q = _fresh()
    toks = torch.zeros(1, 5, dtype=torch.long)

    def cache(b=1, dtype=BF):
        return R.new_cache(q, b, R.CTX, dtype)

    with pytest.raises(ValueError, match="tokens: on cpu, expected a GPU tensor"):
        q.prefill_native(toks, cache(), 0)
    with pytest.raises(ValueError, match="expected \\[B, S\\]"):
        q.prefill_native(toks[0], cache(), 0)
    with pytest.raises(ValueError, match="tokens: dtype"):
        q.prefill_native(toks.int(), cache(), 0)
    with pytest.raises(ValueError, match="start 158 \\+ 5 tokens > context 160"):
        q.prefill_native(toks, cache(), 158)
    with pytest.raises(ValueError, match="expected a host int"):
        q.prefill_native(toks, cache(), torch.zeros(1, dtype=torch.long))
    with pytest.raises(ValueError, match="v cache of layer 0: dtype"):
        q.prefill_native(toks, [(k, v.float()) for k, v in cache()], 0)
    kv = [(k.transpose(1, 2).contiguous().transpose(1, 2), v) for k, v in cache()]
    with pytest.raises(ValueError, match="not contiguous"):
        q.prefill_native(toks, kv, 0)
    q.layers[0].wqkv.scale = q.layers[0].wqkv.scale.half()
    with pytest.raises(ValueError, match="layers.0.wqkv.scale: dtype"):
        q.prefill_native(toks, cache(), 0)
    q = _fresh()
    q.cfg = LlamaConfig(**{**vars(q.cfg), "vocab": 500})
    with pytest.raises(ValueError, match="vocab 500 not a multiple of 64"):
        q.prefill_native(toks, cache(), 0)
    tiny = LlamaFp8.from_llama(Llama(LlamaConfig.tiny()))
    with pytest.raises(ValueError, match="head_dim 32"):
        tiny.prefill_native(toks, tiny.new_kv_cache(1, 64), 0)


def test_c2_dequantized_is_the_fp8_model():
    """dequantized(): a bf16 Llama holding scale * e4m3(code) exactly, the embedding and norms as they were."""
    q = Q.fp8_model(0)
    d = Q.dequantized(0)
    src = R.model(0)
    assert isinstance(d, Llama) and all(p.dtype == BF for p in d.parameters())
    assert torch.equal(d.embed.weight, src.embed.weight.to(BF)) and torch.equal(d.norm.weight, src.norm.weight.to(BF))
    for ql, dl, sl in zip(q.layers, d.layers, src.layers):
        assert torch.equal(dl.norm1.weight, sl.norm1.weight.to(BF))
        for fp8, lin, orig in ((ql.wqkv, dl.attn.wqkv, sl.attn.wqkv), (ql.w2, dl.w2, sl.w2)):
            assert torch.equal(lin.weight.to(F64), Q.TABLE[fp8.codes.long()] * fp8.scale.to(F64)[:, None])
            assert bool(((lin.weight.float() - orig.weight).abs() <= 2.0 ** -4 * orig.weight.abs()
                         + fp8.scale[:, None] * 2.0 ** -10).all())
    n8 = sum(b.numel() * b.element_size() for b in q.buffers())
    n16 = sum(p.numel() * 2 for p in src.parameters())
    assert n8 < 0.6 * n16 + src.embed.weight.numel()


# ---- C3 / C4 -----------------------------------------------------------------------------

def test_c3_exact_cases_are_sound():
    """Every partial sum of every case, in any order, is an integer below 2^24
    (exact in fp32), and the expected output is finite."""
    assert len(Q.EXACT_CASES) == len(set(Q.EXACT_CASES))
    assert {b for b, _, _ in Q.EXACT_CASES} == {1, 2, 3, 4, 8}
    for case in Q.EXACT_CASES:
        x, codes, scale = Q.exact_case(*case)
        assert x.shape == (case[0], case[2]) and codes.shape == (case[1], case[2])
        w = Q.TABLE[codes.long()]
        assert bool((w == w.round()).all()) and w.abs().max() <= 8 and x.float().abs().max() <= 4
        assert bool((torch.frexp(scale)[0] == 0.5).all()) and scale.min() >= 2.0 ** -3 and scale.max() <= 2.0 ** 3
        assert bool((scale[1:] != scale[:-1]).all())
        _, mag = Q.exact_sums(x, codes)
        assert mag.max().item() < 2 ** 24, case
        assert bool(torch.isfinite(Q.exact_expected(x, codes, scale).float()).all()), case


def test_c4_exact_cases_catch_mistakes():
    """Each wrong decoding or indexing changes at least one output element of every case."""
    for case in Q.EXACT_CASES:
        x, codes, scale = Q.exact_case(*case)
        want = Q.exact_expected(x, codes, scale)
        wrong = Q.mistakes(x, codes, scale)
        assert ("batch rows swapped" in wrong) == (case[0] > 1)
        for name, got in wrong.items():
            assert not torch.equal(got, want), (case, name)
