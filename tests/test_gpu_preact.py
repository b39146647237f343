"""The "post" epilogue (native/kernels/conv_gemm.hip): producers of a tensor that
only a projection block reads store it already through that block's entry
BN+ReLU, and the block's shortcut and conv1 run without a prologue.  Every
check is bit for bit against the old form -- the raw tensor and the same two
convs with pro= -- because the post epilogue rounds as the prologue does and
the LDS-DMA and prologue kernels share MFMA sequence and K order.

The convs on a pre-activated tensor run with splitk=False, as the runner calls
them: the prologue form never runs split-K, whose reduce would sum the fp32
partials of the K ranges in another order."""
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


def _pro(c, seed):
    return _f((c,), seed, 0.5, 1.5), _f((c,), seed + 1)


def _eye(c):
    return torch.eye(c).reshape(c, c, 1, 1).to(torch.bfloat16).cuda().contiguous(memory_format=CL)


def _same(got, ref):
    assert got.shape == ref.shape and got.is_contiguous(memory_format=CL)
    torch.testing.assert_close(got, ref, atol=0, rtol=0)


def _check_consumers(C, p, y, pro, convs):
    """Each (w, bias, act, stride) on the pre-activated p equals the same conv
    with pro= on the raw y bit for bit, and both match the fp32 reference."""
    for w, bias, act, stride in convs:
        new = C.conv2d(p, w, bias, stride=stride, act=act, splitk=False)
        old = C.conv2d(y, w, bias, stride=stride, act=act, pro=pro)
        _same(new, old)
        ref = C.conv2d_ref(y, w, bias, stride=stride, act=act, pro=pro)
        torch.testing.assert_close(new.float(), ref, **TOL)
        torch.testing.assert_close(old.float(), ref, **TOL)


@pytest.mark.parametrize("nhw", [(3, 64, 61), (1, 9, 10), (1, 351, 339)])
def test_stem_pool_post(C, nhw):
    n, h, w = nhw
    x = _t((n, 3, h, w), 41)
    ws2d = C.stem_weight_s2d(_t((64, 3, 7, 7), 42, scale=(2.0 / 147) ** 0.5))
    pro = _pro(64, 43)
    y = C.stem_pool(x, ws2d)
    p = C.stem_pool(x, ws2d, post=pro)
    assert p is not None
    _same(p, C.conv2d(y, _eye(64), pro=pro))
    sc = _t((256, 64, 1, 1), 45, scale=(2.0 / 64) ** 0.5)
    w1 = _t((64, 64, 1, 1), 46, scale=(2.0 / 64) ** 0.5)
    _check_consumers(C, p, y, pro, [(sc, None, "none", 1), (w1, _f((64,), 47), "relu", 1)])


def _boundary_convs(cout, seed):
    """The projection block behind a Cout-wide boundary: stride-2 shortcut
    Cout -> 2 Cout and conv1 Cout -> Cout / 2 with bias + ReLU."""
    sc = _t((2 * cout, cout, 1, 1), seed, scale=(2.0 / cout) ** 0.5)
    w1 = _t((cout // 2, cout, 1, 1), seed + 1, scale=(2.0 / cout) ** 0.5)
    return [(sc, None, "none", 2), (w1, _f((cout // 2,), seed + 2), "relu", 1)]


@pytest.mark.parametrize("case", [(2, 64, 19, 17, 1), (2, 128, 21, 19, 2), (3, 128, 9, 9, 1), (1, 64, 7, 5, 1)])
def test_conv23_post(C, case):
    n, c, h, w, stride = case
    x = _t((n, c, h, w), 21)
    w2 = _t((c, c, 3, 3), 22, scale=(2.0 / (9 * c)) ** 0.5)
    b2 = _f((c,), 23)
    w3 = _t((4 * c, c, 1, 1), 24, scale=(2.0 / c) ** 0.5)
    oh, ow = C.out_hw(h, w, 3, stride, 1)
    res = _t((n, 4 * c, oh, ow), 25)
    pro = _pro(4 * c, 26)
    y = C.conv23(x, w2, b2, w3, res, stride=stride)
    p = C.conv23(x, w2, b2, w3, res, stride=stride, post=pro)
    assert p is not None
    _check_consumers(C, p, y, pro, _boundary_convs(4 * c, 28))


CONV3 = [(2, 256, 9, 11, 1024), (5, 512, 6, 6, 2048)]  # the second: M % 64 != 0


@pytest.mark.parametrize("tile_m", [64, 128])
@pytest.mark.parametrize("case", CONV3, ids=lambda c: "x".join(map(str, c)))
def test_conv3_residual_post(C, case, tile_m):
    from vgpu.native import load_kernels
    n, c, h, w, cout = case
    x = _t((n, c, h, w), 31)
    w3 = _t((cout, c, 1, 1), 32, scale=(2.0 / c) ** 0.5)
    res = _t((n, cout, h, w), 33)
    pro = _pro(cout, 34)
    lib = load_kernels()
    lib.vgpu_conv_set_tile_m(tile_m)
    try:
        y = C.conv2d(x, w3, residual=res)
        p = C.conv2d(x, w3, residual=res, post=pro)
        assert p is not None
        _check_consumers(C, p, y, pro, _boundary_convs(cout, 36))
    finally:
        lib.vgpu_conv_set_tile_m(0)


def test_conv3_residual_post_splitk(C):
    """The producer forced onto split-K (two K ranges): the reduce kernel
    applies the post epilogue to the rounded sum, so the consumers see the
    same bits as with the raw split-K output and pro=."""
    n, c, h, w, cout = CONV3[1]
    x = _t((n, c, h, w), 31)
    w3 = _t((cout, c, 1, 1), 32, scale=(2.0 / c) ** 0.5)
    res = _t((n, cout, h, w), 33)
    pro = _pro(cout, 34)
    C.set_splitk(3)
    try:
        assert C.load_kernels().vgpu_conv2d_workspace(n, h, w, c, cout, 1, 1, 0, 0) > 0
        y = C.conv2d(x, w3, residual=res)
        p = C.conv2d(x, w3, residual=res, post=pro)
    finally:
        C.set_splitk(-1)
    assert p is not None  # applied in the reduce, not declined
    _check_consumers(C, p, y, pro, _boundary_convs(cout, 36))


def _randomised(m):
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            mod.running_mean.uniform_(-0.1, 0.1)
            mod.running_var.uniform_(0.5, 1.5)
            mod.weight.data.uniform_(0.5, 1.5)
            mod.bias.data.uniform_(-0.1, 0.1)
    return m.to(torch.bfloat16).to(memory_format=CL)


@pytest.mark.parametrize("net,shapes", [("resnet_v2_50", [(2, 3, 128, 128), (1, 3, 96, 80)]),
                                        ("resnet_v2_152", [(1, 3, 64, 64)])])
def test_runner_preact_equals_prologue_form(gpu_build, net, shapes):
    """Whole runner: preact=True (pre-activated stage boundaries) against
    preact=False (the prologue on the projection blocks' convs), same logits
    bit for bit.  ResNet-V2-152 at 64² has one-tile boundaries."""
    from vgpu.models import resnet
    torch.manual_seed(0)
    m = _randomised(getattr(resnet, net)().cuda().eval())
    new = resnet.FusedResNetV2Inference(m, preact=True)
    old = resnet.FusedResNetV2Inference(m, preact=False)
    for i, shape in enumerate(shapes):
        x = _t(shape, 50 + i)
        got, ref = new(x), old(x)
        assert torch.isfinite(ref.float()).all()
        torch.testing.assert_close(got, ref, atol=0, rtol=0)
