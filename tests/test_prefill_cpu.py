"""The native Llama prefill without a GPU: its argument checks refuse, before
the library is loaded, what the kernels cannot take (C1); the inputs and the
bound of the GPU attention test tell the right arithmetic from a mask off by
one and from a wrong grouped-query mapping (C2); and the CPU references of the
end-to-end test are sound (C3)."""
import pytest
import torch

import _decode_ref as R
import _prefill_ref as PR
from vgpu.models.llama import Llama, LlamaConfig, rope_tables

BF = R.BF


@pytest.fixture
def P(monkeypatch):
    """vgpu.ops.prefill with a library loader that fails the test."""
    from vgpu.ops import decode as D, prefill as mod

    def no_load():
        raise AssertionError("the native library was loaded before the arguments were checked")
    monkeypatch.setattr(mod, "load_kernels", no_load)
    monkeypatch.setattr(D, "load_kernels", no_load)
    return mod


def _rope_args(B=2, S=5, H=4, KVH=2, hd=64, ctx=160, max_seq=256):
    cos, sin = rope_tables(LlamaConfig(dim=hd, heads=1, max_seq=max_seq))
    return dict(qkv=torch.zeros(B * S, (H + 2 * KVH) * hd, dtype=BF), cos=cos, sin=sin, start=0,
                q_out=torch.zeros(B, S, H, hd, dtype=BF), kcache=torch.zeros(B, KVH, ctx, hd, dtype=BF),
                vcache=torch.zeros(B, KVH, ctx, hd, dtype=BF))


def _attn_args(B=2, S=5, H=4, KVH=2, hd=64, ctx=160):
    return dict(q=torch.zeros(B, S, H, hd, dtype=BF), kcache=torch.zeros(B, KVH, ctx, hd, dtype=BF),
                vcache=torch.zeros(B, KVH, ctx, hd, dtype=BF), start=0, out=torch.zeros(B, S, H * hd, dtype=BF),
                scale=0.125)


def _noncontig(t):
    u = t.transpose(1, 2).contiguous().transpose(1, 2)
    assert u.shape == t.shape and not u.is_contiguous()
    return u


def test_c1_rope_kv_write_seq_checks(P):
    def refuses(match, **change):
        with pytest.raises(ValueError, match=match):
            P.rope_kv_write_seq(**{**_rope_args(), **change})
    a = _rope_args()
    refuses("qkv: shape", qkv=a["qkv"][:, :-64].contiguous())
    refuses("vcache: shape", vcache=a["vcache"][:, :, :100].contiguous())
    refuses("kcache: not contiguous", kcache=_noncontig(a["kcache"]))
    refuses("q_out: dtype", q_out=a["q_out"].float())
    refuses("cos: dtype", cos=a["cos"].to(BF))
    refuses(r"start 156 \+ 5 tokens > context 160", start=156)
    refuses(r"start 0 \+ 5 tokens > max_seq 4", cos=a["cos"][:4].contiguous(), sin=a["sin"][:4].contiguous())
    refuses("start -1 < 0", start=-1)
    refuses("expected a host int", start=torch.zeros(1, dtype=torch.long))
    with pytest.raises(ValueError, match="head_dim 32"):
        P.rope_kv_write_seq(**_rope_args(hd=32))
    refuses("qkv: on cpu, expected a GPU tensor")  # everything else in order: the device comes last


def test_c1_attn_prefill_checks(P):
    def refuses(match, **change):
        with pytest.raises(ValueError, match=match):
            P.attn_prefill(**{**_attn_args(), **change})
    a = _attn_args()
    refuses("out: shape", out=a["out"].view(2, 5, 4, 64))
    refuses("q / kcache: shapes", q=a["q"].view(10, 4, 64))
    refuses("vcache: not contiguous", vcache=_noncontig(a["vcache"]))
    refuses("q: dtype", q=a["q"].float())
    refuses(r"start 156 \+ 5 tokens > context 160", start=156)
    refuses("scale", scale=0.0)
    with pytest.raises(ValueError, match="9 query heads per kv head"):
        P.attn_prefill(**_attn_args(H=18, KVH=2))
    refuses("q: on cpu, expected a GPU tensor")


def test_c1_gemm_checks(P):
    def z(*shape, dtype=BF):
        return torch.zeros(shape, dtype=dtype)
    with pytest.raises(ValueError, match="K 72"):
        P.gemm(z(4, 72), z(64, 72), z(4, 64))
    with pytest.raises(ValueError, match="N 96"):
        P.gemm(z(4, 64), z(96, 64), z(4, 96))
    with pytest.raises(ValueError, match="w: shape"):
        P.gemm(z(4, 64), z(128, 128), z(4, 128))
    with pytest.raises(ValueError, match="y: shape"):
        P.gemm(z(4, 64), z(128, 64), z(4, 64))
    with pytest.raises(ValueError, match="x: not contiguous"):
        P.gemm(z(64, 4).t(), z(128, 64), z(4, 128))
    with pytest.raises(ValueError, match="w: dtype"):
        P.gemm(z(4, 64), z(128, 64, dtype=torch.float32), z(4, 128))
    with pytest.raises(ValueError, match="x: on cpu, expected a GPU tensor"):
        P.gemm(z(4, 64), z(128, 64), z(4, 128))
    # 32-bit byte offsets in the GEMM kernels: 8 x 8192 rows of Llama-3's w13 do not fit, 8192 rows do
    assert P.gemm_reason(8 * 8192, 4096, 28672) is not None
    assert P.gemm_reason(8192, 4096, 28672) is None and P.gemm_reason(8192, 14336, 4096) is None
    assert P.gemm_reason(37449, 4096, 28672) is None and P.gemm_reason(37450, 4096, 28672) is not None


def test_c1_prefill_native_checks(P):
    assert hasattr(Llama, "prefill_native")
    m = R.model_as(0, BF)
    prompt, _ = PR.p4_tokens(0, 1)

    def cache(ctx=R.CTX, dtype=BF, b=1):
        return R.new_cache(m, b, ctx, dtype)
    with pytest.raises(ValueError, match="tokens: shape"):
        m.prefill_native(prompt[0], cache())
    with pytest.raises(ValueError, match="kv_caches: 1 layers"):
        m.prefill_native(prompt, cache()[:1])
    with pytest.raises(ValueError, match="k cache of layer 0: shape"):
        m.prefill_native(prompt, cache(b=2))
    kv = [(_noncontig(k), v) for k, v in cache()]
    with pytest.raises(ValueError, match="k cache of layer 0: not contiguous"):
        m.prefill_native(prompt, kv)
    with pytest.raises(ValueError, match="k cache of layer 0: dtype"):
        m.prefill_native(prompt, cache(dtype=torch.float32))
    with pytest.raises(ValueError, match="dtype"):
        R.model_as(0, torch.float32).prefill_native(prompt, cache())
    with pytest.raises(ValueError, match=r"start 124 \+ 37 tokens > context 160"):
        m.prefill_native(prompt, cache(), 124)
    with pytest.raises(ValueError, match=r"start 220 \+ 37 tokens > max_seq 256"):
        m.prefill_native(prompt, cache(ctx=300), 220)
    with pytest.raises(ValueError, match="expected a host int"):
        m.prefill_native(prompt, cache(), torch.zeros(1, dtype=torch.long))
    with pytest.raises(ValueError, match="tokens: dtype"):
        m.prefill_native(prompt.int(), cache())
    tiny = Llama(LlamaConfig.tiny()).to(BF).eval()
    with pytest.raises(ValueError, match="head_dim 32"):
        tiny.prefill_native(prompt[:, :4], tiny.new_kv_cache(1, 16))
    for cfg, why in ((LlamaConfig(vocab=512, dim=96, layers=1, heads=1, kv_heads=1, ffn=256, max_seq=64), "dim 96"),
                     (LlamaConfig(vocab=512, dim=128, layers=1, heads=2, kv_heads=1, ffn=1032, max_seq=64),
                      "ffn 1032"),
                     (LlamaConfig(vocab=500, dim=128, layers=1, heads=2, kv_heads=1, ffn=256, max_seq=64),
                      "vocab 500")):
        bad = Llama(cfg).to(BF).eval()
        with pytest.raises(ValueError, match=f"{why} not a multiple of 64"):
            bad.prefill_native(prompt[:, :4], bad.new_kv_cache(1, 16))
    with pytest.raises(ValueError, match="tokens: on cpu, expected a GPU tensor"):
        m.prefill_native(prompt, cache())


def test_c1_shape_reason():
    from vgpu.ops.prefill import shape_reason
    assert shape_reason(1, 2048, 0, 32, 8, 128, 8192) is None
    assert shape_reason(9, 1, 159, 8, 8, 64, 160) is None
    for case, why in (((0, 1, 0, 32, 8, 128, 8), "batch 0"), ((1, 0, 0, 32, 8, 128, 8), "0 prompt tokens"),
                      ((1, 1, -1, 32, 8, 128, 8), "start -1"), ((1, 4, 5, 32, 8, 128, 8), "> context 8"),
                      ((1, 1, 0, 32, 8, 96, 8), "head_dim 96"), ((1, 1, 0, 32, 5, 128, 8), "not a multiple"),
                      ((1, 1, 0, 32, 2, 128, 8), "16 query heads"), ((70000, 1, 0, 8, 8, 64, 8), "batch 70000"),
                      ((8, 2 ** 20, 0, 32, 8, 128, 2 ** 20), "32-bit index")):
        assert why in shape_reason(*case), case


@pytest.mark.parametrize("case", PR.P2_CASES, ids=PR.case_id)
def test_c2_emulation_against_the_bound(case):
    """The kernel's arithmetic class stays inside 2^-7 A on P2's inputs, a mask
    off by one in either direction does not, nor does the h % KVH mapping."""
    B, H, KVH, hd, S, start, ctx = case
    q, k, v, scale = PR.p2_inputs(case)
    ref, A = PR.attn64(q, k, v, start, scale)
    good = PR.excess(PR.emulate(q, k, v, start, scale), ref, A)
    assert good <= 1.0, good
    worst = [good]
    if start + S >= 2:
        for shift in (1, -1):
            bad = PR.excess(PR.emulate(q, k, v, start, scale, mask_shift=shift), ref, A)
            assert bad > 1.0, (shift, bad)
            worst.append(bad)
    if KVH > 1 and H > KVH:  # with one query head per kv head, h % KVH is h // (H / KVH): nothing to tell apart
        bad = PR.excess(PR.emulate(q, k, v, start, scale, wrong_gqa=True), ref, A)
        assert bad > 1.0, bad
        worst.append(bad)
    print(PR.case_id(case), " ".join(f"{x:.3g}" for x in worst))


@pytest.mark.parametrize("ci,b", [(0, 1), (0, 2), (1, 1), (1, 2)])
def test_c3_eager_reference(ci, b):
    ref = PR.p4_reference(ci, b)
    for key in ("f64", "bf16", "f64_dec", "bf16_dec"):
        assert torch.isfinite(ref[key]).all(), key
    assert ref["f64"].shape == (b, R.CONFIGS[ci].vocab) and ref["f64_dec"].shape == (3, b, R.CONFIGS[ci].vocab)
    assert 0.0 < ref["e_eager"] < 0.1 and 0.0 < ref["e_eager_dec"] < 0.1
    for k, v in ref["f64_kv"]:
        assert bool((k[:, :, PR.PROMPT:] == R.FILL).all()) and bool((v[:, :, PR.PROMPT:] == R.FILL).all())
        assert not bool((k[:, :, :PR.PROMPT] == R.FILL).any())
