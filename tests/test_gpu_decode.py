"""native/kernels/decode.hip and Llama.decode_native against fp64 on the CPU.

References: G1-G4 compute the kernel's own formula in fp64 from the bf16
inputs; G5 / G6 use decode_static of the fp64 model on the CPU (equal to
`forward`, test_decode_cpu.py C1).  No bound is taken from the kernels.

Every buffer a kernel writes through a direct library call is allocated with
16 further rows of 0xFF bytes, and those rows must be untouched afterwards.
Cache rows beyond `pos` hold 64.0: finite, so a reference that read them would
stay finite, and 20 or more standard deviations from any k or v, so a kernel
that read them is far outside every bound.

Which test fails for which mistake (argued from decode.hip):
  * GQA head mapping wrong (query head h not reading kv head h // (H/KVH)):
    G3 at (H, KVH) = (8, 2); K and V differ per kv head.
  * mask off by one (`<` instead of `<=` pos): G3 at pos = 0 (no key at all:
    zeros instead of v[0]) and at c - 1, c, c + 1 around the chunk boundary c.
  * reading past pos: G3 and G5 through the 64.0 fill.
  * an empty chunk turning into NaN (exp(-inf - -inf)): G3 at ctx = 1024,
    pos = 0 (seven empty chunks) and ctx = 160, pos <= 127.
  * combine order or weights wrong: G3 at ctx = 160 and 1024 with pos = ctx - 1.
  * interleaved instead of half-split RoPE pairs: G2.
  * cache row index or stride wrong: G2 (every other row bit-identical, guard
    rows intact at pos = ctx - 1, nothing written at pos = ctx).
  * norm taken from the unrounded sum x + delta: G1's reference is the norm of
    the rounded h (the difference is up to half a bf16 ulp of h, which moves y
    across its own bound for a share of the elements); G5's caches and logits.
  * pos read on the host, or anything else frozen at capture: G6.
"""
import ctypes

import pytest
import torch

import _decode_ref as R
from vgpu.models.llama import LlamaConfig, rope_tables

pytestmark = pytest.mark.gpu

BF, F64 = R.BF, R.F64
HEADS = [(4, 2), (8, 2)]
EPS = 1e-5


@pytest.fixture(scope="module")
def lib(gpu_build):
    from vgpu.ops import decode as D
    return D._lib()


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


# ---- G1 add_rmsnorm --------------------------------------------------------------------

@pytest.mark.parametrize("with_delta", [False, True])
@pytest.mark.parametrize("rows", [1, 3, 8])
@pytest.mark.parametrize("dim", [512, 4096])
def test_g1_add_rmsnorm(lib, dim, rows, with_delta):
    g = _gen(dim + rows)
    x = torch.randn(rows, dim, generator=g).to(BF)
    delta = torch.randn(rows, dim, generator=g).to(BF) if with_delta else None
    w = (torch.rand(dim, generator=g) + 0.5).to(BF)
    xg, yg = Guarded(rows, dim, fill=x), Guarded(rows, dim)
    dg = delta.cuda() if with_delta else None
    wg = w.cuda()
    assert lib.vgpu_add_rmsnorm(xg.ptr, _ptr(dg), _ptr(wg), yg.ptr, rows, dim, EPS, _stream()) == 0
    torch.cuda.synchronize()
    h = (x.float() + delta.float()).to(BF) if with_delta else x
    assert torch.equal(xg.t.cpu(), h)
    h64 = h.to(F64)
    ref = h64 * torch.rsqrt(h64.pow(2).mean(-1, keepdim=True) + EPS) * w.to(F64)
    _bound_ok(yg.t.cpu(), ref, 2.0 ** -8, 1e-6, "y")
    assert xg.intact() and yg.intact()


# ---- G2 rope_kv_write ------------------------------------------------------------------

def _tables(hd, max_seq=256):
    return rope_tables(LlamaConfig(dim=hd, heads=1, max_seq=max_seq))  # fp32 [max_seq, hd / 2], on the CPU


def _rope64(x, cos, sin):
    """x [..., hd] bf16 -> fp64 rotation (first half pairs with second half) and its bound's |x1| + |x2|."""
    x1, x2 = x.to(F64).chunk(2, dim=-1)
    c, s = cos.to(F64), sin.to(F64)
    mag = x1.abs() + x2.abs()
    return torch.cat([x1 * c - x2 * s, x1 * s + x2 * c], dim=-1), torch.cat([mag, mag], dim=-1)


@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("H,KVH", HEADS)
@pytest.mark.parametrize("B", [1, 3])
def test_g2_rope_kv_write(lib, B, H, KVH, hd):
    ctx, max_seq = 160, 256
    cos, sin = _tables(hd, max_seq)
    cg, sg = cos.cuda(), sin.cuda()
    fill = torch.full((B * KVH * ctx, hd), R.FILL, dtype=BF)
    kc, vc = Guarded(B * KVH * ctx, hd, fill=fill), Guarded(B * KVH * ctx, hd, fill=fill)
    pos = torch.zeros(1, dtype=torch.long, device="cuda")
    for p in (0, 1, 63, 64, 159, 160):  # 160 = ctx: outside, nothing may be written
        qkv = torch.randn(B, (H + 2 * KVH) * hd, generator=_gen(p + hd + H)).to(BF)
        qg = Guarded(B * H, hd)
        k_before, v_before = kc.t.cpu().view(B, KVH, ctx, hd), vc.t.cpu().view(B, KVH, ctx, hd)
        pos.fill_(p)
        rc = lib.vgpu_rope_kv_write(_ptr(qkv.cuda()), _ptr(cg), _ptr(sg), _ptr(pos), qg.ptr, kc.ptr, vc.ptr, B, H,
                                    KVH, hd, ctx, max_seq, _stream())
        assert rc == 0
        torch.cuda.synchronize()
        k_after, v_after = kc.t.cpu().view(B, KVH, ctx, hd), vc.t.cpu().view(B, KVH, ctx, hd)
        assert kc.intact() and vc.intact() and qg.intact(), p
        if p >= ctx:
            assert torch.equal(k_after, k_before) and torch.equal(v_after, v_before)
            continue
        q, k, v = qkv.view(B, H + 2 * KVH, hd).split([H, KVH, KVH], dim=1)
        for name, got, src in (("q", qg.t.cpu().view(B, H, hd), q), ("k", k_after[:, :, p], k)):
            ref, mag = _rope64(src, cos[p], sin[p])
            _bound_ok(got, ref, 2.0 ** -8, 2.0 ** -20 * mag, f"{name} at pos {p}")
        assert torch.equal(v_after[:, :, p], v), p
        others = torch.arange(ctx) != p
        assert torch.equal(k_after[:, :, others], k_before[:, :, others]), p
        assert torch.equal(v_after[:, :, others], v_before[:, :, others]), p


# ---- G3 attn_decode --------------------------------------------------------------------

def _attn64(q, k, v, pos, scale):
    """q [B, H, hd], k / v [B, KVH, ctx, hd] (bf16) -> fp64 [B, H, hd] over keys 0..pos."""
    rep = q.shape[1] // k.shape[1]
    k64 = k[:, :, :pos + 1].to(F64).repeat_interleave(rep, dim=1)
    v64 = v[:, :, :pos + 1].to(F64).repeat_interleave(rep, dim=1)
    s = torch.einsum("bhd,bhkd->bhk", q.to(F64), k64) * scale
    return torch.einsum("bhk,bhkd->bhd", torch.softmax(s, dim=-1), v64)


@pytest.mark.parametrize("ctx", [1, 64, 160, 1024])
@pytest.mark.parametrize("hd", [64, 128])
@pytest.mark.parametrize("H,KVH", HEADS)
def test_g3_attn_decode(lib, H, KVH, hd, ctx):
    c = lib.vgpu_attn_decode_chunk(ctx)
    assert c >= 1 and lib.vgpu_attn_decode_chunk(ctx) == c
    positions = sorted({p for p in (0, ctx - 1, c - 1, c, c + 1) if 0 <= p < ctx})
    scale = hd ** -0.5
    pos = torch.zeros(1, dtype=torch.long, device="cuda")
    for B in (1, 3):
        g = _gen(ctx + hd + H + B)
        q = torch.randn(B, H, hd, generator=g).to(BF)
        k_all = torch.randn(B, KVH, ctx, hd, generator=g).to(BF)
        v_all = torch.randn(B, KVH, ctx, hd, generator=g).to(BF)
        need = lib.vgpu_attn_decode_workspace(B, H, hd, ctx)
        chunks = (ctx + c - 1) // c
        per = need // (4 * B * H * chunks)  # floats per (row, head, chunk) partial: m, l, o[hd]
        assert need == 4 * B * H * chunks * per and per >= hd + 2
        qg = q.cuda()
        for p in positions:
            k, v = k_all.clone(), v_all.clone()
            k[:, :, p + 1:] = R.FILL
            v[:, :, p + 1:] = R.FILL
            kg, vg = k.cuda(), v.cuda()
            pos.fill_(p)
            outs = []
            for _ in range(2):
                out = Guarded(B, H * hd)
                ws = Guarded(B * H * chunks, per, torch.float32)
                rc = lib.vgpu_attn_decode(_ptr(qg), _ptr(kg), _ptr(vg), _ptr(pos), out.ptr, ws.ptr, need, B, H, KVH,
                                          hd, ctx, scale, _stream())
                assert rc == 0
                torch.cuda.synchronize()
                assert out.intact() and ws.intact(), (B, p)
                outs.append(out.t.cpu().view(B, H, hd))
            assert torch.equal(outs[0], outs[1]), (B, p)
            ref = _attn64(q, k, v, p, scale)
            extra = 4 * ctx * 2.0 ** -23 * v[:, :, :p + 1].to(F64).abs().max().item()
            _bound_ok(outs[0], ref, 2.0 ** -8, extra, f"B {B} pos {p}")
            if p == 0:
                assert torch.equal(outs[0], v[:, :, 0].repeat_interleave(H // KVH, dim=1)), B


def test_g3_shapes_refused(lib):
    """vgpu_decode_supported's rules, and the Python check that mirrors them."""
    from vgpu.ops.decode import shape_reason
    cases = [(b, 32, 8, 128, 1024) for b in range(0, 10)] + [(1, 32, 8, hd, 8) for hd in (32, 64, 96, 128, 256)]
    cases += [(1, 32, 5, 128, 8), (1, 32, 2, 128, 8), (1, 32, 4, 128, 8), (1, 8, 8, 64, 1), (1, 8, 2, 64, 0)]
    for case in cases:
        assert bool(lib.vgpu_decode_supported(*case)) == (shape_reason(*case) is None), case


# ---- G4 swiglu -------------------------------------------------------------------------

@pytest.mark.parametrize("ffn", [1024, 14336])
@pytest.mark.parametrize("B", [1, 8])
def test_g4_swiglu(lib, B, ffn):
    gu = (torch.randn(B, 2 * ffn, generator=_gen(B + ffn)) * 2).to(BF)
    y = Guarded(B, ffn)
    assert lib.vgpu_swiglu(_ptr(gu.cuda()), y.ptr, B, ffn, _stream()) == 0
    torch.cuda.synchronize()
    g, u = gu.to(F64).chunk(2, dim=-1)
    _bound_ok(y.t.cpu(), g * torch.sigmoid(g) * u, 2.0 ** -8, 2.0 ** -20 * (g * u).abs(), "y")
    assert y.intact()


# ---- G5 end to end ---------------------------------------------------------------------

def _cache_ok(kv, ref, written, what):
    """Rows in `written` against the fp64 run's, every other row still 64.0.

    Layer 0: within one bf16 ulp.  Its input is the embedding row, the same
    bits in every run, so k and v differ from fp64 only by the roundings of the
    norm, the GEMV output and the rotation.  An element is a sum of hundreds of
    products, so its error does not shrink with its own size: the ulp is taken
    at the largest magnitude the reference holds in those rows (2^-7 of it).

    Deeper layers: their input carries a whole layer's bf16 error, and no bf16
    run stays within an ulp of fp64 there (the eager bf16 run on the CPU is off
    by up to 2.4 ulp in these cases).  The bound is the one the logits have,
    twice the eager run's own error against fp64 on the same rows."""
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


@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("ci", [0, 1])
def test_g5_decode_native_end_to_end(gpu_build, ci, B):
    """e_native <= 2 e_eager, both the largest logit error against the fp64 run
    over all 22 steps.  Measured on an MI355X, e_eager / e_native: config 0
    B 1 0.0137 / 0.0134, B 2 0.0144 / 0.0112; config 1 B 1 0.0356 / 0.0337,
    B 2 0.0218 / 0.0186 (logits up to 2.5)."""
    ref = R.reference(ci, B)
    toks = R.tokens(ci, B)
    m = R.model_as(ci, BF, "cuda")
    kv = R.new_cache(m, B, R.CTX, BF, "cuda")
    got = R.run_steps(m, m.decode_native, toks[:20], kv, R.STEPS[:20], "cuda")
    # a row is written once: the reference caches after step 19 are the final ones without rows 158, 159
    _cache_ok(kv, ref, torch.arange(20), "after 20 steps")
    got = torch.cat([got, R.run_steps(m, m.decode_native, toks[20:], kv, R.STEPS[20:], "cuda")])
    _cache_ok(kv, ref, torch.tensor(R.STEPS), "after all steps")
    assert got.shape == ref["f64"].shape and torch.isfinite(got).all()
    e_native = (got - ref["f64"]).abs().max().item()
    e_20 = (got[:20] - ref["f64"][:20]).abs().max().item()
    e_eager_20 = (ref["bf16"][:20] - ref["f64"][:20]).abs().max().item()
    print(f"config {ci} B {B}: e_eager {ref['e_eager']:.4e} e_native {e_native:.4e} "
          f"(positions 0..19 only: {e_eager_20:.4e} / {e_20:.4e}), max |logit| {ref['f64'].abs().max().item():.3f}")
    assert e_native <= 2 * ref["e_eager"]


# ---- G6 graph replay -------------------------------------------------------------------

def test_g6_graph_replay(gpu_build):
    ci, B = 0, 1
    toks = R.tokens(ci, B)[:20].cuda()
    m = R.model_as(ci, BF, "cuda")
    kv_plain = R.new_cache(m, B, R.CTX, BF, "cuda")
    pos = torch.zeros(1, dtype=torch.long, device="cuda")
    want = []
    for p in range(20):
        pos.fill_(p)
        want.append(m.decode_native(toks[p], kv_plain, pos).clone())

    kv = R.new_cache(m, B, R.CTX, BF, "cuda")
    tok = toks[0].clone()
    pos.fill_(0)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        for _ in range(2):
            m.decode_native(tok, kv, pos)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = m.decode_native(tok, kv, pos)
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
