"""The halo form of the fused tails' phase 1 (conv23_kernel<..., HALO>,
native/kernels/conv_gemm.hip): conv2's nine taps read their A fragments from one
halo image of the tile's input range in LDS, not from nine gathers.  The K order
is the ring form's, so every result has the ring form's bits; on exact-integer
operands both equal a float64 reference.  Shapes the rule (conv_plan.h,
conv23_halo_ok) does not take run the ring: stride 2, images too wide for the
region, and C = 128, whose halo form measured inside the ring's own spread on the
flagship and was removed (profiles/r11/tail_halo/README.md) -- the C = 128 cases
stay here and assert that."""
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

CL = torch.channels_last
BF = torch.bfloat16

# (n, h, w): one partial tile; exact tiles; tiles straddling images (several per
# XCD numbering); a one-row image; a one-column image (every horizontal tap is
# padding); every output pixel a corner
SHAPES = [(1, 7, 5), (1, 16, 16), (3, 23, 21), (2, 1, 9), (2, 9, 1), (2, 2, 2)]
FORMS = [("conv23", 64), ("conv23", 128), ("post", 64), ("post", 128), ("conv231", 64), ("conv231", 128),
         ("conv231_sc", 64)]


@pytest.fixture(scope="module")
def C(gpu_build):
    from vgpu.ops import conv
    return conv


@pytest.fixture(scope="module")
def lib(gpu_build):
    from vgpu.native import load_kernels
    return load_kernels()


def _t(shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(BF).cuda().contiguous(memory_format=CL)


def _f(shape, seed, lo=-0.5, hi=0.5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(shape, generator=g) * (hi - lo) + lo).cuda().contiguous()


def _operands(n, c, h, w, stride=1):
    """As tests/test_gpu_shortcut_tail.py builds them; h and xp are ReLU outputs
    (they hold exact zeros, as pre-activated tensors do)."""
    oh, ow = (h - 1) // stride + 1, (w - 1) // stride + 1
    return dict(
        h=_t((n, c, h, w), 61).clamp_min(0).contiguous(memory_format=CL),
        w2=_t((c, c, 3, 3), 62, scale=(2.0 / (9 * c)) ** 0.5),
        b2=_f((c,), 63),
        w3=_t((4 * c, c, 1, 1), 64, scale=(2.0 / c) ** 0.5),
        res=_t((n, 4 * c, oh, ow), 72),
        xp=_t((n, 64, h, w), 65).clamp_min(0).contiguous(memory_format=CL),
        wsc=_t((4 * c, 64, 1, 1), 66, scale=(2.0 / 64) ** 0.5),
        w1n=_t((c, 4 * c, 1, 1), 67, scale=(2.0 / (4 * c)) ** 0.5),
        b1n=_f((c,), 68),
        pro_n=(_f((4 * c,), 69, 0.5, 1.5), _f((4 * c,), 70)),
        post=(_f((4 * c,), 73, 0.5, 1.5), _f((4 * c,), 74)),
    )


def _run(C, form, o, stride=1):
    """The form's outputs as a tuple of tensors."""
    if form == "conv23":
        return (C.conv23(o["h"], o["w2"], o["b2"], o["w3"], o["res"], stride=stride),)
    if form == "post":
        return (C.conv23(o["h"], o["w2"], o["b2"], o["w3"], o["res"], stride=stride, post=o["post"]),)
    if form == "conv231":
        return tuple(C.conv231(o["h"], o["w2"], o["b2"], o["w3"], o["res"], o["w1n"], o["b1n"], o["pro_n"],
                               stride=stride))
    assert form == "conv231_sc"
    return tuple(C.conv231(o["h"], o["w2"], o["b2"], o["w3"], None, o["w1n"], o["b1n"], o["pro_n"],
                           stride=stride, shortcut=(o["xp"], o["wsc"])))


def _on_off(C, lib, form, o, stride=1):
    """(outputs with the halo switched on, halo launches they made, outputs with it off)."""
    try:
        lib.vgpu_conv23_set_halo(1)
        before = lib.vgpu_conv23_halo_launches()
        on = _run(C, form, o, stride)
        launches = lib.vgpu_conv23_halo_launches() - before
        lib.vgpu_conv23_set_halo(0)
        before = lib.vgpu_conv23_halo_launches()
        off = _run(C, form, o, stride)
        assert lib.vgpu_conv23_halo_launches() == before
    finally:
        lib.vgpu_conv23_set_halo(-1)
    torch.cuda.synchronize()
    return on, launches, off


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form,c", FORMS)
def test_halo_equals_ring(C, lib, form, c, shape):
    n, h, w = shape
    o = _operands(n, c, h, w)
    assert (o["h"] == 0).any()
    on, launches, off = _on_off(C, lib, form, o)
    assert launches == (1 if c == 64 else 0)  # one call, one launch, in the halo form; C = 128 keeps the ring
    assert len(on) == len(off) == (1 if form in ("conv23", "post") else 2)
    for got, ref in zip(on, off):
        assert got is not None and got.shape == ref.shape and got.is_contiguous(memory_format=CL)
        assert torch.isfinite(ref.float()).all()
        torch.testing.assert_close(got, ref, atol=0, rtol=0)


# ---- exact integers ---------------------------------------------------------------

def _ints(shape, seed, lo, hi, dtype=BF, cl=True):
    g = torch.Generator(device="cpu").manual_seed(seed)
    t = torch.randint(lo, hi + 1, shape, generator=g).to(dtype)
    return t.cuda().contiguous(memory_format=CL) if cl else t.cuda().contiguous()


def _pow2(shape, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (2.0 ** torch.randint(-1, 2, shape, generator=g).float()).cuda().contiguous()  # 0.5, 1, 2


def _int_operands(n, c, h, w):
    """x and every weight from {-1, 0, 1}; biases and shifts small integers, scales powers of two."""
    return dict(
        h=_ints((n, c, h, w), 81, -1, 1),
        w2=_ints((c, c, 3, 3), 82, -1, 1),
        b2=_ints((c,), 83, -3, 3, torch.float32, False),
        w3=_ints((4 * c, c, 1, 1), 84, -1, 1),
        res=_ints((n, 4 * c, h, w), 85, -4, 4),
        xp=_ints((n, 64, h, w), 86, -1, 1),
        wsc=_ints((4 * c, 64, 1, 1), 87, -1, 1),
        w1n=_ints((c, 4 * c, 1, 1), 88, -1, 1),
        b1n=_ints((c,), 89, -3, 3, torch.float32, False),
        pro_n=(_pow2((4 * c,), 90), _ints((4 * c,), 91, -2, 2, torch.float32, False)),
        post=(_pow2((4 * c,), 92), _ints((4 * c,), 93, -2, 2, torch.float32, False)),
    )


def _bf16(t):
    """float64 -> bf16 (round to nearest even) -> float64; exact through fp32 for |t| < 2^24 in half-integer steps."""
    assert float(t.abs().max()) < 2 ** 23
    return t.float().to(BF).double()


_REFS = {}


def _int_reference(n, c, h, w):
    """float64 on the CPU, rounded to bf16 where the kernel rounds: h2, the
    shortcut, y, the post value / the next block's prologue value, h1.
    Computed once per shape and width and shared by the forms."""
    key = (n, c, h, w)
    if key in _REFS:
        return _REFS[key]
    o = _int_operands(n, c, h, w)
    d = {k: (tuple(t.double().cpu() for t in v) if isinstance(v, tuple) else v.double().cpu()) for k, v in o.items()}
    h2 = (F.conv2d(d["h"], d["w2"], d["b2"], padding=1)).clamp_min(0)
    # the premise: conv2's sums stay at or below 256, so h2 is exact in bf16
    assert float(h2.abs().max()) <= 256 and float(F.conv2d(d["h"], d["w2"], padding=1).abs().max()) <= 256
    h2 = _bf16(h2)
    c3 = F.conv2d(h2, d["w3"])
    assert float(c3.abs().max()) + 64 + 4 < 2 ** 24  # every fp32 sum exact in any order
    sc = _bf16(F.conv2d(d["xp"], d["wsc"]))

    def act(y, ss):
        return _bf16((y * ss[0].view(1, -1, 1, 1) + ss[1].view(1, -1, 1, 1)).clamp_min(0))

    def next_h1(y):
        p = act(y, d["pro_n"])
        s = F.conv2d(p, d["w1n"])
        assert float(F.conv2d(p.abs(), d["w1n"].abs()).max()) < 2 ** 23
        return _bf16((s + d["b1n"].view(1, -1, 1, 1)).clamp_min(0))

    y = _bf16(c3 + d["res"])
    y_sc = _bf16(c3 + sc)
    ref = {"conv23": (y,), "post": (act(y, d["post"]),), "conv231": (y, next_h1(y)),
           "conv231_sc": (y_sc, next_h1(y_sc))}
    _REFS[key] = (o, ref)
    return _REFS[key]


@pytest.mark.parametrize("shape", [(3, 23, 21), (2, 9, 1)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("form,c", FORMS)
def test_exact_integers(C, lib, form, c, shape):
    n, h, w = shape
    o, ref = _int_reference(n, c, h, w)
    before = lib.vgpu_conv23_halo_launches()
    try:
        lib.vgpu_conv23_set_halo(1)
        got = _run(C, form, o)
    finally:
        lib.vgpu_conv23_set_halo(-1)
    torch.cuda.synchronize()
    assert lib.vgpu_conv23_halo_launches() - before == (1 if c == 64 else 0)
    assert len(got) == len(ref[form])
    for g, r in zip(got, ref[form]):
        assert torch.equal(g.cpu().double(), r), float((g.cpu().double() - r).abs().max())


# ---- declines -------------------------------------------------------------------------

@pytest.mark.parametrize("why,shape,stride", [("stride=2", (2, 10, 9), 2), ("too wide", (1, 2, 400), 1)])
@pytest.mark.parametrize("form,c", [("conv23", 64), ("conv23", 128), ("post", 128), ("conv231", 64), ("conv231", 128)])
def test_declines_run_the_ring(C, lib, form, c, why, shape, stride):
    n, h, w = shape
    o = _operands(n, c, h, w, stride)
    on, launches, off = _on_off(C, lib, form, o, stride)
    assert launches == 0
    for got, ref in zip(on, off):
        assert got is not None and torch.isfinite(ref.float()).all()
        torch.testing.assert_close(got, ref, atol=0, rtol=0)


# ---- runner ----------------------------------------------------------------------------

def _randomised(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.uniform_(-0.1, 0.1)
            mod.running_var.uniform_(0.5, 1.5)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.uniform_(-0.1, 0.1)
    return m.to(BF).to(memory_format=CL)


class _Tails:
    """Counts the runner's fused-tail calls while it runs: stride 1 at C = 64 (the
    halo form's), and the others."""

    def __init__(self, conv, monkeypatch):
        self.stride1 = self.other = 0
        for name in ("conv23", "conv231"):
            real = getattr(conv, name)

            def counted(*a, _real=real, **kw):
                out = _real(*a, **kw)
                if out is not None:
                    if kw.get("stride", 1) == 1 and a[0].shape[1] == 64:
                        self.stride1 += 1
                    else:
                        self.other += 1
                return out

            monkeypatch.setattr(conv, name, counted)


@pytest.mark.parametrize("net,shapes", [("resnet_v2_50", [(2, 3, 128, 128), (1, 3, 96, 80)]),
                                        ("resnet_v2_152", [(1, 3, 64, 64)])])
def test_runner_halo_equals_ring(C, lib, monkeypatch, net, shapes):
    """Whole runner: logits with the halo form equal logits with VGPU_CONV23_HALO=0
    bit for bit, and every stride-1 tail of stage 1 took the halo form (stage 1 of
    these inputs is at most 32 pixels wide)."""
    from vgpu.models import resnet
    torch.manual_seed(0)
    m = _randomised(getattr(resnet, net)().cuda().eval())
    runner = resnet.FusedResNetV2Inference(m)
    tails = _Tails(C, monkeypatch)
    monkeypatch.delenv("VGPU_CONV23_HALO", raising=False)
    for i, shape in enumerate(shapes):
        x = _t(shape, 50 + i)
        tails.stride1 = tails.other = 0
        before = lib.vgpu_conv23_halo_launches()
        got = runner(x)
        took = lib.vgpu_conv23_halo_launches() - before
        assert tails.stride1 == 3 and tails.other >= 4  # b0-b2; stage 2's tails
        assert took == tails.stride1
        monkeypatch.setenv("VGPU_CONV23_HALO", "0")
        before = lib.vgpu_conv23_halo_launches()
        ref = runner(x)
        assert lib.vgpu_conv23_halo_launches() == before
        monkeypatch.delenv("VGPU_CONV23_HALO")
        assert torch.isfinite(ref.float()).all()
        torch.testing.assert_close(got, ref, atol=0, rtol=0)
