"""scripts/roofline.py plan(): block 0's projection shortcut is part of its
fused tail row (conv23_kernel<128, 64, NEXT, SC>), CPU only."""
import importlib.util
import os

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _roofline():
    spec = importlib.util.spec_from_file_location("roofline", os.path.join(REPO, "scripts", "roofline.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def test_block0_shortcut_row_is_merged_into_its_tail():
    r = _roofline()
    p = r.plan(50, 346)
    names = [k[0] for k in p]
    assert len(p) == 42  # one dispatch fewer than with a stand-alone b0 shortcut
    assert "b0 shortcut 1x1 (pre-activated input)" not in names
    assert names[1:3] == ["b0 conv1 1x1 (pre-activated input)", "b0 shortcut+conv2+conv3+next conv1"]
    # the other projection shortcuts (stride 2) keep their rows
    assert sum("shortcut 1x1" in n for n in names) == 3
    m, e = 50 * 87 * 87, 2
    _, flops, nbytes = p[2]
    # shortcut (K 64 -> 256) + conv2 (3x3, 64) + conv3 (64 -> 256) + next conv1 (256 -> 64)
    assert flops == 2 * m * (64 * 256 + 9 * 64 * 64 + 64 * 256 + 256 * 64)
    # in: x' and h (64 wide each); out: y (256 wide) and h1 (64 wide); the four weight tensors
    assert nbytes == e * (m * 64 + m * 64 + m * 256 + m * 64 + 64 * 256 + 9 * 64 * 64 + 64 * 256 + 256 * 64)
    # against the unmerged plan: same FLOPs; the 256-wide shortcut output is
    # neither written nor read back (x' was and is read once for the shortcut)
    assert sum(k[1] for k in p) == 1004191404800
    assert sum(k[2] for k in p) == 5521192624 - 2 * m * 256 * e


def test_resnet152_plan_takes_the_same_path():
    r = _roofline()
    names = [k[0] for k in r.plan(50, 346, (3, 8, 36, 3))]
    assert "b0 shortcut+conv2+conv3+next conv1" in names
    assert sum("shortcut 1x1" in n for n in names) == 3
