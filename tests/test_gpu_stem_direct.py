"""The fused stem on the image itself (vgpu_stem_pool_x_nhwc) and its bands.

stem_pool_kernel walks bands of pooled rows (native/kernels/stem_plan.h) and,
in its direct form, gathers the space-to-depth input from x [N][H][W][3] inside
the kernel.  Neither changes a bit of the result: every comparison here is
atol = 0, rtol = 0 against maxpool3s2(stem_conv(x, w)), which runs the
space-to-depth kernel, the LDS-DMA conv and the max-pool kernel.
"""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last
# (N, H, W): the smallest shapes that reach each edge
SHAPES = [
    (1, 1, 1),      # one stem row, one pooled row
    (1, 2, 3),
    (1, 9, 10),
    (2, 11, 12),    # OH even: the last pooled row has no third stem row
    (3, 64, 61),    # odd W: rows are only 2-byte aligned
    (2, 37, 351),   # OW = 176: the widest row, the last subtile
    (1, 12, 352),
    (300, 5, 6),    # more bands than workgroups: the band loop
]


@pytest.fixture(scope="module")
def C(gpu_build):
    from vgpu.ops import conv
    yield conv
    conv.set_stem_band(0)


def _t(shape, seed, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(torch.bfloat16).cuda().contiguous(memory_format=CL)


def _f(shape, seed, lo=-0.5, hi=0.5):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(shape, generator=g) * (hi - lo) + lo).cuda().contiguous()


def _eye(c):
    return torch.eye(c).reshape(c, c, 1, 1).to(torch.bfloat16).cuda().contiguous(memory_format=CL)


def _same(got, ref):
    assert got.shape == ref.shape and got.is_contiguous(memory_format=CL)
    torch.testing.assert_close(got, ref, atol=0, rtol=0)


def _ph(h):
    return ((h - 1) // 2 + 1 - 1) // 2 + 1


_CASES = {}


def _case(C, nhw):
    """x, w, post parameters and the two references of a shape, computed once by unchanged kernels."""
    if nhw not in _CASES:
        n, h, w = nhw
        x = _t((n, 3, h, w), 41)
        ws2d = C.stem_weight_s2d(_t((64, 3, 7, 7), 42, scale=(2.0 / 147) ** 0.5))
        pro = (_f((64,), 43, 0.5, 1.5), _f((64,), 44))
        ref = C.maxpool3s2(C.stem_conv(x, ws2d))
        ref_post = C.conv2d(ref, _eye(64), pro=pro)  # as tests/test_gpu_preact.py::test_stem_pool_post
        _CASES[nhw] = (x, ws2d, pro, ref, ref_post)
    return _CASES[nhw]


def _direct(C, x, ws2d, post, guard=3):
    """The C entry on x with NaN-filled output and guard rows around it; (rc, y or None)."""
    from vgpu.native import load_kernels
    n, _, h, w = x.shape
    oh, ow = C.out_hw(h, w, 7, 2, 3)
    ph, pw = C.out_hw(oh, ow, 3, 2, 1)
    row = pw * 64
    buf = torch.full(((n * ph + 2 * guard) * row,), float("nan"), dtype=torch.bfloat16, device="cuda")
    y = buf[guard * row:(guard + n * ph) * row]
    vp = ctypes.c_void_p
    qs, qt = (vp(post[0].data_ptr()), vp(post[1].data_ptr())) if post is not None else (None, None)
    rc = load_kernels().vgpu_stem_pool_x_nhwc(vp(x.data_ptr()), vp(ws2d.data_ptr()), vp(y.data_ptr()), qs, qt,
                                              n, h, w, vp(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    if rc != 0:
        assert torch.isnan(buf).all()  # nothing launched
        return rc, None
    assert torch.isnan(buf[:guard * row]).all() and torch.isnan(buf[(guard + n * ph) * row:]).all()
    return rc, y.view(n, ph, pw, 64).permute(0, 3, 1, 2)


@pytest.mark.parametrize("band", ["heuristic", 1, 2, 3, "PH"])
@pytest.mark.parametrize("nhw", SHAPES)
def test_direct_equals_conv_then_pool(C, nhw, band):
    x, ws2d, pro, ref, ref_post = _case(C, nhw)
    C.set_stem_band({"heuristic": 0, "PH": _ph(nhw[1])}.get(band, band))
    try:
        for post, want in ((None, ref), (pro, ref_post)):
            rc, y = _direct(C, x, ws2d, post)
            assert rc == 0
            assert not torch.isnan(y.float()).any()  # every pooled row written
            _same(y, want)
            _same(C.stem_pool(x, ws2d, post=post), want)
    finally:
        C.set_stem_band(0)


@pytest.mark.parametrize("nhw", [(3, 64, 61), (2, 37, 351)])
def test_x_input_entries_equal_direct(C, nhw):
    """The entries on the space-to-depth tensor run the same banded kernel."""
    x, ws2d, pro, ref, ref_post = _case(C, nhw)
    X = C.stem_space_to_depth(x)
    try:
        for band in (1, 2, _ph(nhw[1])):
            C.set_stem_band(band)
            for post in (None, pro):
                _, y = _direct(C, x, ws2d, post)
                _same(C.stem_pool_s2d(X, ws2d, post=post), y)
    finally:
        C.set_stem_band(0)


def test_too_wide_is_refused(C):
    """OW = 177: the C entry launches nothing; stem_pool gives the two-kernel result, None for post."""
    x, ws2d, pro, ref, _ = _case(C, (1, 8, 353))
    for post in (None, pro):
        rc, y = _direct(C, x, ws2d, post)
        assert rc == -1 and y is None
    _same(C.stem_pool(x, ws2d), ref)
    assert C.stem_pool(x, ws2d, post=pro) is None


def test_image_at_the_end_of_its_allocation(C):
    """Odd W, x ending exactly where its allocation ends: every address the kernel may
    form for a pixel of the image lies inside [x, x + N*H*W*3), checked here on the host
    for the shape, and the result is that of the same image elsewhere."""
    nhw = (3, 64, 61)
    x, ws2d, pro, ref, _ = _case(C, nhw)
    n, h, w = nhw
    numel = n * h * w * 3
    store = torch.empty(numel + 64, dtype=torch.bfloat16, device="cuda")
    tail = store[64:]
    assert tail.data_ptr() + numel * 2 == store.data_ptr() + store.numel() * 2
    assert tail.data_ptr() % 4 == 0 and (w * 3) % 2 == 1  # odd rows start on an odd element: 2-byte aligned only
    tail.copy_(x.permute(0, 2, 3, 1).reshape(-1))
    xe = tail.view(n, h, w, 3).permute(0, 3, 1, 2)
    assert xe.is_contiguous(memory_format=CL)
    # the kernel's loads per tap: elements (r*W + c)*3 .. +2 of an image, for 0 <= r < H, 0 <= c < W
    assert ((h - 1) * w + (w - 1)) * 3 + 2 == h * w * 3 - 1
    rc, y = _direct(C, xe, ws2d, None)
    assert rc == 0
    _same(y, ref)


@pytest.mark.parametrize("model,nhw", [("resnet_v2_50", (2, 64, 61)), ("resnet_v2_152", (1, 40, 40))])
def test_runner_logits_do_not_depend_on_the_stem_path(gpu_build, monkeypatch, model, nhw):
    import vgpu.models.resnet as R
    torch.manual_seed(0)
    m = getattr(R, model)(num_classes=16).cuda().to(torch.bfloat16).to(memory_format=CL).eval()
    x = _t((nhw[0], 3, nhw[1], nhw[2]), 7)
    out = {}
    for preact in (True, False):
        for direct in ("1", "0"):
            monkeypatch.setenv("VGPU_STEM_DIRECT", direct)
            runner = R.FusedResNetV2Inference(m, preact=preact)
            assert runner.stem_direct == (direct == "1")
            out[preact, direct] = runner(x)
        torch.testing.assert_close(out[preact, "1"], out[preact, "0"], atol=0, rtol=0)
