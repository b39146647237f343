"""vgpu.ops.loss without a GPU: for every layout `_layout` accepts, the
gradient tensor `_CrossEntropyFn.forward` allocates (`_grad_like`) really
holds element (rows - 1, C - 1) at the strides the kernel writes with.  A
padded-row view used to get a packed [rows, C] gradient from
torch.empty_like, and the kernel, addressing it by the logits' row stride, ran
past its end."""
import pytest
import torch

from vgpu.ops.loss import _grad_like, _layout


def _dense(dtype=torch.float32):
    return torch.zeros(5, 1000, dtype=dtype)


def _padded(dtype=torch.float32):
    return torch.zeros(5, 1024, dtype=dtype)[:, :1000]


def _cl(dtype=torch.float32):
    return torch.zeros(2, 21, 5, 7, dtype=dtype).contiguous(memory_format=torch.channels_last)


def _nchw(dtype=torch.float32):
    return torch.zeros(3, 64, 9, 11, dtype=dtype)


def _one_row_padded(dtype=torch.float32):
    return torch.zeros(1, 1024, dtype=dtype)[:, :1000]


CASES = {"dense": _dense, "padded": _padded, "cl": _cl, "nchw": _nchw, "one_row_padded": _one_row_padded}


def _last_offset(lay):
    """The largest storage offset the kernel touches: element (rows - 1, C - 1)
    by loss.hip's base(row) + c * cstride."""
    rows, c, hw, bs, ps, cs = lay
    row = rows - 1
    return (row // hw) * bs + (row % hw) * ps + (c - 1) * cs


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
@pytest.mark.parametrize("name", list(CASES))
def test_dlogits_holds_what_the_kernel_writes(name, dtype):
    x = CASES[name](dtype)
    lay = _layout(x)
    assert lay is not None, "a layout the op takes natively"
    rows, c = lay[0], lay[1]
    d = _grad_like(x)
    assert d.shape == x.shape and d.dtype == x.dtype and d.stride() == x.stride()
    have = d.untyped_storage().nbytes() // d.element_size() - d.storage_offset()
    assert _last_offset(lay) < have, (lay, have)
    # and every (row, class) is its own element of d: the layout's offsets are d's
    r = torch.tensor([0, rows // 2, rows - 1])
    for row in r.tolist():
        for cls in (0, c - 1):
            off = (row // lay[2]) * lay[3] + (row % lay[2]) * lay[4] + cls * lay[5]
            if x.dim() == 2:
                want = row * d.stride(0) + cls * d.stride(1)
            else:
                hw_w = x.shape[3]
                b, pix = divmod(row, lay[2])
                want = b * d.stride(0) + cls * d.stride(1) + (pix // hw_w) * d.stride(2) + (pix % hw_w) * d.stride(3)
            assert off == want


def test_padded_view_is_what_empty_like_packs():
    """The reason for _grad_like: empty_like of a padded view is compact."""
    x = _padded()
    assert x.stride() == (1024, 1)
    assert torch.empty_like(x).stride() == (1000, 1)
    assert _grad_like(x).stride() == (1024, 1)
    lay = _layout(x)
    assert lay == (5, 1000, 5, 0, 1024, 1)
    assert _last_offset(lay) >= torch.empty_like(x).numel()  # where the old allocation ended


def test_layout_refuses_what_the_kernel_cannot_address():
    assert _layout(torch.zeros(5, 1000).t()) is None                # column stride != 1
    assert _layout(torch.zeros(5, 8)[:, ::2]) is None
    assert _layout(torch.zeros(1, 4).expand(5, 4)) is None          # overlapping rows (stride 0 < C)
    assert _layout(torch.zeros(2, 21, 5, 8)[:, :, :, :7]) is None   # pixels of an image not one run
    assert _layout(torch.zeros(5)) is None
