"""attn_decode (native/kernels/decode.hip) and attn_prefill (prefill.hip) held
bit for bit to the int64 references of tests/_attn_exact.py: scores that
select, values that count, so that the kernel must store bf16(S / n) whatever
its split.  tests/test_attn_exact_cpu.py proves on every case that a single
key lost or counted twice changes a stored value.

Every call goes to the library directly, into outputs and a workspace that are
followed by 16 sentinel rows of 0xFF bytes; each call runs twice and the two
results must be equal.  Cache rows beyond the visible range hold K = 0 and
V = 64.0: a kernel that read one would select it.

The ids of test_decode_exact name the instantiation: hd 64 / 128 x G = 1 .. 8
are the 16 attn_decode_partial_kernel<HD, G>; ctx 8192, 8193 and 12345 are the
chunks of 128, 192 and 256 keys (asserted through vgpu_attn_decode_chunk)."""
import ctypes

import pytest
import torch

import _attn_exact as AE

pytestmark = pytest.mark.gpu

BF = AE.BF


@pytest.fixture(scope="module")
def lib(gpu_build):
    from vgpu.ops import decode as D
    from vgpu.ops import prefill as P
    D._lib()
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
    return ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- decode ----------------------------------------------------------------------------

def _decode_twice(lib, case, qg, kg, vg, pos, scale):
    """Two runs into fresh guarded buffers; both results, equal, as [B, H, hd] on the CPU."""
    B, H, KVH, hd, ctx = case
    plan = case.plan
    need = lib.vgpu_attn_decode_workspace(B, H, hd, ctx)
    per = need // (4 * B * H * plan.chunks)  # floats per (row, head, chunk) partial
    assert need == 4 * B * H * plan.chunks * per and per >= hd + 2
    outs = []
    for _ in range(2):
        out = Guarded(B, H * hd)
        ws = Guarded(B * H * plan.chunks, per, torch.float32)
        rc = lib.vgpu_attn_decode(_ptr(qg), _ptr(kg), _ptr(vg), _ptr(pos), out.ptr, ws.ptr, need, B, H, KVH, hd, ctx,
                                  scale, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert out.intact() and ws.intact()
        outs.append(out.t.cpu().view(B, H, hd))
    assert torch.equal(outs[0], outs[1])
    return outs[0]


@pytest.mark.parametrize("case", AE.DECODE_CASES, ids=AE.decode_id)
def test_decode_exact(lib, case):
    plan = case.plan
    assert lib.vgpu_attn_decode_chunk(case.ctx) == plan.c
    if case.ctx in AE.GROWN:
        assert plan.c == AE.GROWN[case.ctx]
    inp = AE.decode_inputs(case)
    qg, kg, vg = inp["q"].cuda(), inp["k"].cuda(), inp["v"].cuda()
    pos = torch.zeros(1, dtype=torch.long, device="cuda")
    for p in AE.decode_positions(plan):
        kp, vp = AE.tempt(kg, vg, p + 1)
        pos.fill_(p)
        got = _decode_twice(lib, case, qg, kp, vp, pos, inp["scale"])
        n, S, want = AE.decode_ref(inp, p)
        assert torch.equal(got, want), (p, (got != want).nonzero()[:4].tolist())


@pytest.mark.parametrize("case", [AE.DCase(B, 2 * AE.BATCH_G[hd], 2, hd, 160) for hd in (64, 128) for B in (1, 3)],
                         ids=AE.decode_id)
def test_decode_contract(lib, case):
    """*pos < 0: zeros.  *pos >= ctx: all ctx keys, nothing beyond the cache."""
    inp = AE.decode_inputs(case)
    qg = inp["q"].cuda()
    pos = torch.zeros(1, dtype=torch.long, device="cuda")
    kt, vt = AE.tempt(inp["k"], inp["v"], 0)  # every row tempts
    pos.fill_(-1)
    got = _decode_twice(lib, case, qg, kt.cuda(), vt.cuda(), pos, inp["scale"])
    assert torch.equal(got, torch.zeros_like(got))
    want = AE.decode_ref(inp, case.ctx - 1)[2]
    kc = Guarded(case.B * case.KVH * case.ctx, case.hd, fill=inp["k"].view(-1, case.hd))
    vc = Guarded(case.B * case.KVH * case.ctx, case.hd, fill=inp["v"].view(-1, case.hd))
    for p in (case.ctx, case.ctx + 7):
        pos.fill_(p)
        assert torch.equal(AE.decode_ref(inp, p)[2], want)
        assert torch.equal(_decode_twice(lib, case, qg, kc.t, vc.t, pos, inp["scale"]), want), p


@pytest.mark.parametrize("hd", [64, 128])
def test_rope_kv_write_contract(lib, hd):
    """vgpu_rope_kv_write writes nothing at *pos < 0 and at *pos >= max_seq with
    max_seq < ctx (no table row); at max_seq - 1 it writes that cache row."""
    B, H, KVH, ctx, max_seq = 2, 4, 2, 160, 96
    g = torch.Generator().manual_seed(hd)
    cos, sin = torch.rand(max_seq, hd // 2, generator=g).cuda(), torch.rand(max_seq, hd // 2, generator=g).cuda()
    qkv = torch.randn(B, (H + 2 * KVH) * hd, generator=g).to(BF).cuda()
    fill = torch.randn(B * KVH * ctx, hd, generator=g).to(BF)
    kc, vc = Guarded(B * KVH * ctx, hd, fill=fill), Guarded(B * KVH * ctx, hd, fill=fill)
    pos = torch.zeros(1, dtype=torch.long, device="cuda")

    def write(p):
        qg = Guarded(B * H, hd)
        pos.fill_(p)
        rc = lib.vgpu_rope_kv_write(_ptr(qkv), _ptr(cos), _ptr(sin), _ptr(pos), qg.ptr, kc.ptr, vc.ptr, B, H, KVH, hd,
                                    ctx, max_seq, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert kc.intact() and vc.intact() and qg.intact(), p
        return qg

    for p in (-1, max_seq, max_seq + 3, ctx - 1, ctx):
        qg = write(p)
        assert torch.equal(kc.t.cpu(), fill) and torch.equal(vc.t.cpu(), fill), p
        assert bool((qg.raw == 0xFF).all()), p  # q is not written either
    write(max_seq - 1)
    k_after, v_after = kc.t.cpu().view(B, KVH, ctx, hd), vc.t.cpu().view(B, KVH, ctx, hd)
    others = torch.arange(ctx) != max_seq - 1
    before = fill.view(B, KVH, ctx, hd)
    assert torch.equal(k_after[:, :, others], before[:, :, others])
    assert torch.equal(v_after[:, :, others], before[:, :, others])
    v_new = qkv.cpu().view(B, H + 2 * KVH, hd)[:, H + KVH:]
    assert torch.equal(v_after[:, :, max_seq - 1], v_new)
    assert not torch.equal(k_after[:, :, max_seq - 1], before[:, :, max_seq - 1])


# ---- prefill ---------------------------------------------------------------------------

@pytest.mark.parametrize("case", AE.PREFILL_CASES, ids=AE.prefill_id)
def test_prefill_exact(lib, case):
    B, H, KVH, hd, S, start, ctx = case
    inp = AE.prefill_inputs(case)
    qg, kg, vg = inp["q"].cuda(), inp["k"].cuda(), inp["v"].cuda()
    outs = []
    for _ in range(2):
        out = Guarded(B * S, H * hd)
        rc = lib.vgpu_attn_prefill(_ptr(qg), _ptr(kg), _ptr(vg), out.ptr, B, S, start, H, KVH, hd, ctx, inp["scale"],
                                   _stream())
        assert rc == 0
        torch.cuda.synchronize()
        assert out.intact()
        outs.append(out.t.cpu().view(B, S, H, hd))
    assert torch.equal(outs[0], outs[1])
    want = AE.prefill_ref(inp)[2]
    assert torch.equal(outs[0], want), (outs[0] != want).nonzero()[:4].tolist()
