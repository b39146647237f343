"""Plan and launch agree on the GPU: three rows of scripts/conv_plan_trace.py's table
whose kernel the setters fix (so the CU count of the test machine does not matter)
run through vgpu_conv2d_nhwc_ws; the halo-launch counter moves exactly when the
golden trace names the halo kernel, the workspace is the golden one, and the output
is the exact integer result.  Numerics of every family are covered elsewhere."""
import ctypes
import json
from pathlib import Path

import pytest
import torch

pytestmark = pytest.mark.gpu

CL = torch.channels_last
GOLDEN = json.loads((Path(__file__).parent / "golden" / "conv_plan_parent.json").read_text())

ROWS = [
    # 3x3 C 64 -> 128, forced halo BM 256 on W = 16: the halo kernel
    (dict(H=8, W=16, C=64, Cout=128, knobs=dict(halo=2)), "conv_halo_kernel<256, 128, 384, 0>"),
    # the same on W = 48: no halo tile fits, the LDS-DMA kernel takes it
    (dict(H=48, W=48, C=64, Cout=128, knobs=dict(halo=2)), "conv_glds_kernel<3, "),
    # forced halo and three forced splits with a workspace: split-K wins
    (dict(H=8, W=8, C=512, Cout=128, ws="exact", knobs=dict(halo=1, splitk=3)),
     "conv_glds_kernel<3, 64, 128, false, 0, 0, true, false>"),
]


def _golden_row(want: dict) -> dict:
    want = {"ep": "conv", "KS": 3, "pad": 1, "stride": 1, "pro": False, "res": False, "ws": "none", **want}
    hits = [r for r in GOLDEN["256"] if all(r["spec"][k] == v for k, v in want.items())]
    assert len(hits) == 1, want
    return hits[0]


@pytest.mark.parametrize("want,first_kernel", ROWS, ids=["halo", "halo-falls-back", "splitk-over-halo"])
def test_launch_follows_plan(gpu_build, want, first_kernel):
    from vgpu.native import load_kernels
    from vgpu.ops import conv as C
    row = _golden_row(want)
    s = row["spec"]
    assert row["rc"] == 0 and row["launches"][0][0].startswith(first_kernel)
    # the family is the same at 8 CUs (the fallback's tile height is not: it follows the CU count)
    assert [r for r in GOLDEN["8"] if r["spec"] == s][0]["launches"][0][0].startswith(first_kernel)
    g = torch.Generator(device="cpu").manual_seed(s["H"] + s["C"])
    x = torch.randint(-2, 3, (1, s["C"], s["H"], s["W"]), generator=g).to(torch.bfloat16).cuda()
    w = torch.randint(-2, 3, (s["Cout"], s["C"], 3, 3), generator=g).to(torch.bfloat16).cuda()
    x, w = x.contiguous(memory_format=CL), w.contiguous(memory_format=CL)
    y = torch.empty((1, s["Cout"], s["H"], s["W"]), dtype=torch.bfloat16, device="cuda", memory_format=CL)
    lib = load_kernels()
    setters = dict(halo=lib.vgpu_conv_set_halo, splitk=lib.vgpu_conv_set_splitk)
    vp = ctypes.c_void_p
    try:
        for k, v in s["knobs"].items():
            setters[k](v)
        need = lib.vgpu_conv2d_workspace(1, s["H"], s["W"], s["C"], s["Cout"], 3, 1, 1, 0)
        assert need == row["ws"]
        ws = torch.empty(max(need, 4) // 4, dtype=torch.float32, device="cuda") if s["ws"] == "exact" else None
        before = lib.vgpu_conv_halo_launches()
        rc = lib.vgpu_conv2d_nhwc_ws(vp(x.data_ptr()), vp(w.data_ptr()), vp(y.data_ptr()), None, None, None, None, 1,
                                     s["H"], s["W"], s["C"], s["Cout"], 3, 1, 1, 0,
                                     vp(ws.data_ptr()) if ws is not None else None, need if ws is not None else 0,
                                     vp(torch.cuda.current_stream().cuda_stream))
        halo_ran = lib.vgpu_conv_halo_launches() - before
    finally:
        for k in s["knobs"]:
            setters[k](-1)
    assert rc == row["rc"]
    assert halo_ran == sum("conv_halo_kernel" in name for name, _, _ in row["launches"])
    # fp32 sums of these integers are exact in any order (|sum| <= 4 * 9 * 512 < 2^24), split or not;
    # the kernel rounds them once to bf16
    assert torch.equal(y.float(), C.conv2d_ref(x, w, stride=1, padding=1).to(torch.bfloat16).float())
