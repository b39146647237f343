"""Block 0's projection shortcut computed inside its fused tail
(conv23_kernel<128, 64, NEXT, SC>, native/kernels/conv_gemm.hip): the kernel
runs the K = 64 shortcut GEMM on the pre-activated block input per conv3 chunk,
rounds it to bf16 where the stand-alone conv stores it and adds it in fp32 to
the conv3 accumulators, so y and the next block's h1 equal, bit for bit, the
stand-alone shortcut conv followed by conv231 with that tensor as residual."""
import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last
TOL = dict(atol=3e-2, rtol=2e-2)  # the project's bf16 conv tolerance (tests/test_gpu_conv.py)


@pytest.fixture(scope="module")
def C(gpu_build):
    from vgpu.ops import conv
    return conv


def _t(shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).cuda().contiguous(memory_format=CL)


def _f(shape, seed, lo=-0.5, hi=0.5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(shape, generator=g) * (hi - lo) + lo).cuda().contiguous()


def _operands(n, c, h, w, csc=64):
    """The tail's operands for a W = c block whose shortcut reads csc channels;
    xp is a ReLU output (it holds exact zeros, as a pre-activated tensor does)."""
    return dict(
        h=_t((n, c, h, w), 61),
        w2=_t((c, c, 3, 3), 62, scale=(2.0 / (9 * c)) ** 0.5),
        b2=_f((c,), 63),
        w3=_t((4 * c, c, 1, 1), 64, scale=(2.0 / c) ** 0.5),
        xp=_t((n, csc, h, w), 65).clamp_min(0).contiguous(memory_format=CL),
        wsc=_t((4 * c, csc, 1, 1), 66, scale=(2.0 / csc) ** 0.5),
        w1n=_t((c, 4 * c, 1, 1), 67, scale=(2.0 / (4 * c)) ** 0.5),
        b1n=_f((c,), 68),
        pro_n=(_f((4 * c,), 69, 0.5, 1.5), _f((4 * c,), 70)),
    )


def _old(C, o, stride=1, sc_stride=1):
    """The separate sequence: the stand-alone shortcut conv, then conv231 on its output."""
    sc = C.conv2d(o["xp"], o["wsc"], stride=sc_stride, splitk=False)
    return C.conv231(o["h"], o["w2"], o["b2"], o["w3"], sc, o["w1n"], o["b1n"], o["pro_n"], stride=stride)


# M = n·h·w rows in 128-row tiles: 35 (one partial tile), 646 (several), 1449
# (11 tiles + 41 rows), 256 (exactly two full tiles)
@pytest.mark.parametrize("case", [(1, 64, 7, 5), (2, 64, 19, 17), (3, 64, 23, 21), (1, 64, 16, 16)],
                         ids=lambda c: "x".join(map(str, c)))
def test_shortcut_in_tail_equals_shortcut_then_tail(C, case):
    n, c, h, w = case
    o = _operands(n, c, h, w)
    assert (o["xp"] == 0).any()
    out = C.conv231(o["h"], o["w2"], o["b2"], o["w3"], None, o["w1n"], o["b1n"], o["pro_n"],
                    shortcut=(o["xp"], o["wsc"]))
    assert out is not None
    y, h1 = out
    y_old, h1_old = _old(C, o)
    for got, ref in ((y, y_old), (h1, h1_old)):
        assert got.shape == ref.shape and got.is_contiguous(memory_format=CL)
        torch.testing.assert_close(got, ref, atol=0, rtol=0)
    # and both forms against fp32, with the bf16 intermediates the kernels round
    h2 = C.conv2d_ref(o["h"], o["w2"], o["b2"], padding=1, act="relu").to(torch.bfloat16).contiguous(memory_format=CL)
    sc = C.conv2d_ref(o["xp"], o["wsc"]).to(torch.bfloat16).contiguous(memory_format=CL)
    y_ref = C.conv2d_ref(h2, o["w3"], residual=sc)
    for got in (y, y_old):
        torch.testing.assert_close(got.float(), y_ref, **TOL)
    h1_ref = C.conv2d_ref(y_old, o["w1n"], o["b1n"], act="relu", pro=o["pro_n"])
    for got in (h1, h1_old):
        torch.testing.assert_close(got.float(), h1_ref, **TOL)


@pytest.mark.parametrize("why", ["W=128", "stride=2", "K=128"])
def test_shortcut_in_tail_declines(C, why):
    """Shapes the variant does not take answer None, launch nothing, and leave
    the buffers fit for the plain sequence, which still gives the old result."""
    c = 128 if why == "W=128" else 64
    stride = 2 if why == "stride=2" else 1
    csc = 128 if why == "K=128" else 64
    n, h, w = 2, 10, 9
    o = _operands(n, c, h, w, csc)
    before = _old(C, o, stride, stride)
    out = C.conv231(o["h"], o["w2"], o["b2"], o["w3"], None, o["w1n"], o["b1n"], o["pro_n"], stride=stride,
                    shortcut=(o["xp"], o["wsc"]))
    assert out is None
    after = _old(C, o, stride, stride)
    for got, ref in zip(after, before):
        torch.testing.assert_close(got, ref, atol=0, rtol=0)


def test_conv231_wants_one_residual_source(C):
    o = _operands(1, 64, 7, 5)
    res = _t((1, 256, 7, 5), 71)
    with pytest.raises(ValueError):
        C.conv231(o["h"], o["w2"], o["b2"], o["w3"], None, o["w1n"], o["b1n"], o["pro_n"])
    with pytest.raises(ValueError):
        C.conv231(o["h"], o["w2"], o["b2"], o["w3"], res, o["w1n"], o["b1n"], o["pro_n"],
                  shortcut=(o["xp"], o["wsc"]))


def _randomised(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.uniform_(-0.1, 0.1)
            mod.running_var.uniform_(0.5, 1.5)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.uniform_(-0.1, 0.1)
    return m.to(torch.bfloat16).to(memory_format=CL)


class _Calls:
    """Counts conv231 calls by form while a runner runs."""

    def __init__(self, conv, monkeypatch):
        self.fused = self.plain = 0
        real = conv.conv231

        def counted(*a, **kw):
            if kw.get("shortcut") is not None:
                self.fused += 1
            else:
                self.plain += 1
            return real(*a, **kw)

        monkeypatch.setattr(conv, "conv231", counted)


@pytest.mark.parametrize("net,shapes", [("resnet_v2_50", [(2, 3, 128, 128), (1, 3, 96, 80)]),
                                        ("resnet_v2_152", [(1, 3, 64, 64)])])
def test_runner_shortcut_in_tail_equals_separate_shortcut(C, monkeypatch, net, shapes):
    """Whole runner, fuse_sc on against off: same logits bit for bit, and the
    fused form is what block 0 ran."""
    from vgpu.models import resnet
    torch.manual_seed(0)
    m = _randomised(getattr(resnet, net)().cuda().eval())
    new = resnet.FusedResNetV2Inference(m, fuse_sc=True)
    old = resnet.FusedResNetV2Inference(m, fuse_sc=False)
    assert new.fuse_sc and not old.fuse_sc
    calls = _Calls(C, monkeypatch)
    for i, shape in enumerate(shapes):
        x = _t(shape, 50 + i)
        calls.fused = 0
        got = new(x)
        assert calls.fused == 1
        ref = old(x)
        assert calls.fused == 1
        assert torch.isfinite(ref.float()).all()
        torch.testing.assert_close(got, ref, atol=0, rtol=0)


def test_runner_fallbacks(C, monkeypatch):
    """Without a pre-activated input (preact=False) or without the fused next
    conv1 (VGPU_FUSE_NEXT=0) block 0 runs the stand-alone shortcut; the env
    switch VGPU_FUSE_SC=0 turns the fusion off.  Logits stay the same bits."""
    from vgpu.models import resnet
    torch.manual_seed(0)
    m = _randomised(resnet.resnet_v2_50().cuda().eval())
    x = _t((1, 3, 96, 80), 51)
    ref = resnet.FusedResNetV2Inference(m, fuse_sc=False)(x)
    calls = _Calls(C, monkeypatch)

    got = resnet.FusedResNetV2Inference(m, preact=False, fuse_sc=True)(x)
    assert calls.fused == 0 and calls.plain > 0
    torch.testing.assert_close(got, ref, atol=0, rtol=0)

    monkeypatch.setenv("VGPU_FUSE_NEXT", "0")
    r = resnet.FusedResNetV2Inference(m, fuse_sc=True)
    monkeypatch.delenv("VGPU_FUSE_NEXT")
    assert not r.fuse_next
    calls.plain = 0
    got = r(x)
    assert calls.fused == 0 and calls.plain == 0
    torch.testing.assert_close(got, ref, atol=0, rtol=0)

    monkeypatch.setenv("VGPU_FUSE_SC", "0")
    r = resnet.FusedResNetV2Inference(m)
    monkeypatch.delenv("VGPU_FUSE_SC")
    assert not r.fuse_sc
    got = r(x)
    assert calls.fused == 0
    torch.testing.assert_close(got, ref, atol=0, rtol=0)
