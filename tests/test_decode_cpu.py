"""Llama decode on the CPU: the reference the GPU decode tests lean on (C1),
and the argument checks of Llama.decode_native, which must refuse what the
native kernels cannot take before any library is loaded (C2)."""
import pytest
import torch

import _decode_ref as R
from vgpu.models.llama import Llama, LlamaConfig


@pytest.mark.parametrize("ci", [0, 1])
def test_c1_decode_static_is_forward_in_fp64(ci):
    """C1: fp64 decode_static (whole cache, positions > pos masked) against fp64
    forward (cache sliced at pos) over positions 0..19: no difference at all."""
    m = R.model_as(ci, R.F64)
    toks = R.tokens(ci, 2)[:20]
    kv_s, kv_f = R.new_cache(m, 2, R.CTX, R.F64), R.new_cache(m, 2, R.CTX, R.F64)
    pos = torch.zeros(1, dtype=torch.long)
    with torch.no_grad():
        for p, t in enumerate(toks):
            pos.fill_(p)
            got = m.decode_static(t, kv_s, pos)
            want = m(t, kv_f, p)
            assert got.shape == want.shape == (2, 1, m.cfg.vocab)
            assert (got - want).abs().max().item() == 0.0, p
    for (ks, vs), (kf, vf) in zip(kv_s, kv_f):
        assert torch.equal(ks, kf) and torch.equal(vs, vf)
        assert bool((ks[:, :, 20:] == R.FILL).all()) and bool((vs[:, :, 20:] == R.FILL).all())


def test_c2_decode_native_refuses_before_loading(monkeypatch):
    """C2: CPU tensors, head_dim 32 and a non-contiguous cache each raise
    ValueError naming that reason, and the native library is never asked for."""
    from vgpu.ops import decode as D

    def no_load():
        raise AssertionError("the native library was loaded before the arguments were checked")
    monkeypatch.setattr(D, "load_kernels", no_load)
    assert hasattr(Llama, "decode_native")
    pos = torch.zeros(1, dtype=torch.long)

    m = R.model_as(0, R.BF)
    tok = R.tokens(0, 1)[0]
    with pytest.raises(ValueError, match="expected a GPU tensor"):
        m.decode_native(tok, R.new_cache(m, 1, R.CTX, R.BF), pos)

    kv = [(k.transpose(1, 2).contiguous().transpose(1, 2), v) for k, v in R.new_cache(m, 1, R.CTX, R.BF)]
    assert kv[0][0].shape == kv[0][1].shape and not kv[0][0].is_contiguous()
    with pytest.raises(ValueError, match="not contiguous"):
        m.decode_native(tok, kv, pos)

    with pytest.raises(ValueError, match="dtype"):
        m.decode_native(tok, R.new_cache(m, 1, R.CTX, torch.float32), pos)
    with pytest.raises(ValueError, match="dtype"):
        R.model_as(0, torch.float32).decode_native(tok, R.new_cache(m, 1, R.CTX, R.BF), pos)
    with pytest.raises(ValueError, match="batch 5"):
        m.decode_native(tok.expand(5, 1), R.new_cache(m, 5, R.CTX, R.BF), pos)

    tiny = Llama(LlamaConfig.tiny()).to(R.BF).eval()
    with pytest.raises(ValueError, match="head_dim 32"):
        tiny.decode_native(tok, tiny.new_kv_cache(1, 64), pos)


def test_c2_shape_rules():
    """The Python shape check states vgpu_decode_supported's rules."""
    from vgpu.ops.decode import shape_reason
    for b in (1, 2, 3, 4, 8):
        assert shape_reason(b, 32, 8, 128, 1024) is None
    assert shape_reason(1, 8, 1, 64, 1) is None
    for bad in ((5, 32, 8, 128, 8), (1, 32, 8, 32, 8), (1, 32, 8, 256, 8), (1, 32, 5, 128, 8), (1, 32, 2, 128, 8),
                (1, 32, 8, 128, 0)):
        assert shape_reason(*bad), bad
