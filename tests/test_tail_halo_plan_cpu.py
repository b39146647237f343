"""The eligibility rule of the fused tails' halo form (native/kernels/conv_plan.h:
conv23_halo_ok and the sizes behind it), without a GPU.

The rule takes C = 64 only.  At C = 128 the sizes below still fit (a ring of two
panels), but on the flagship's 44-wide stage 2 the form did not beat the ring by
more than the ring's own spread (profiles/r11/tail_halo/README.md), so it was
removed and (44, C = 128) keeps the ring.

The header is compiled with g++ behind native/tests/tail_halo_plan_capi.cpp.  The
halo form of conv23_kernel keeps, per 64-channel block, one 128-B LDS row per
input pixel a tile of BM output pixels can read (BM + 2W + 2 of them) plus a zero
row, and a ring of weight panels behind them, all inside the region the ring
form's three (A tile + panel) stages occupy.
"""
from __future__ import annotations

import ctypes
import itertools
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
CS = [0, 32, 64, 96, 128, 192, 256]
STRIDES = [0, 1, 2, 3]
WS = [0, 1, 2, 9, 21, 43, 44, 45, 46, 47, 64, 86, 87, 88, 94, 95, 128, 400, 1 << 20, (1 << 31) - 1]
BMS = [0, 32, 64, 128, 256]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    so = tmp_path_factory.mktemp("tail_halo_plan") / "libtail_halo_plan.so"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-shared", "-fPIC",
                    str(REPO / "native" / "tests" / "tail_halo_plan_capi.cpp"), "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


def test_eligibility_over_c_stride_w_bm(lib):
    """Taken exactly when: stride 1, C = 64, and BM + 2W + 3 rows (the reachable
    pixels and the zero row) fit the block's halo rows."""
    taken = 0
    for c, stride, w, bm in itertools.product(CS, STRIDES, WS, BMS):
        ok = bool(lib.conv23_halo_ok_c(c, stride, w, bm))
        where = (c, stride, w, bm)
        if stride != 1 or c != 64 or w < 1 or bm < 1:
            assert not ok, where
            continue
        rows = lib.conv23_halo_rows_c(c, bm)
        assert ok == (bm + 2 * w + 3 <= rows), where
        if ok:
            taken += 1
            # every tap of every tile pixel lands below the zero row, which is the block's last row
            assert (bm - 1) + 2 * w + 2 < rows - 1, where
            assert rows >= bm + 2 * w + 2 + 1, where
    assert taken > 0


@pytest.mark.parametrize("c", [64, 128])
def test_halo_and_ring_fit_the_ring_forms_region(lib, c):
    bm = lib.conv23_bm_c(c, 0, 0, 0)
    rows, ring = lib.conv23_halo_rows_c(c, bm), lib.conv23_halo_ring_c(c)
    region = lib.conv23_region_c(c, bm)
    assert region == 3 * (bm * 128 + c * 128)  # three stages of an A tile and a weight panel
    assert rows > 0 and rows % 32 == 0  # 256 threads bring in 32 rows per DMA instruction
    assert ring >= 2  # a panel lands while another multiplies
    used = rows * (c // 64) * 128 + ring * c * 128
    assert used == lib.conv23_halo_bytes_c(c, bm)
    assert used <= region
    assert rows * (c // 64) * 128 <= 65536  # 16-bit row addresses


def test_flagship_shapes(lib):
    # stage 1: 87 x 87, C = 64, 128-row tiles: qualifies
    assert lib.conv23_bm_c(64, 1, 0, 1) == 128 and lib.conv23_bm_c(128, 1, 0, 0) == 64
    assert lib.conv23_halo_ok_c(64, 1, 87, 128)
    # stage 2: 44 x 44, C = 128, 64-row tiles: its rows would fit, the measurement removed it
    assert 64 + 2 * 44 + 3 <= lib.conv23_halo_rows_c(128, 64)
    assert not lib.conv23_halo_ok_c(128, 1, 44, 64)
    # the stride-2 tails that end the stages do not
    assert not lib.conv23_halo_ok_c(64, 2, 87, 128)
    assert not lib.conv23_halo_ok_c(128, 2, 44, 64)
    # nor an image too wide for the region
    assert not lib.conv23_halo_ok_c(64, 1, 400, 128)
    assert not lib.conv23_halo_ok_c(128, 1, 400, 64)


def test_conv23_bm_is_unchanged(lib):
    for c in (0, 32, 64, 96, 128, 256):
        for nxt, post, sc in itertools.product((0, 1), repeat=3):
            exists = c in (64, 128) and not (post and nxt) and not (sc and (not nxt or c != 64))
            want = (128 if c == 64 else 64) if exists else 0
            assert lib.conv23_bm_c(c, nxt, post, sc) == want, (c, nxt, post, sc)
