"""Band plan of the fused stem kernel (native/kernels/stem_plan.h), without a GPU.

The header is compiled with g++ behind native/tests/stem_plan_capi.cpp.  A band
is the pooled rows [p0, p1) of one image that a workgroup walks; workgroup g of
`grid` takes the bands g, g + grid, ...  Whatever the rule chooses, the bands
must tile every image exactly and the grid must fit the CUs (LDS admits one
workgroup per CU).
"""
from __future__ import annotations

import ctypes
import shutil
import subprocess
from pathlib import Path

import pytest

REPO = Path(__file__).resolve().parents[1]
NS = [1, 2, 3, 10, 50, 255, 256, 257, 300]
PHS = [1, 2, 3, 5, 32, 87, 88]
CUS = [8, 128, 256]


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("g++ not found")
    so = tmp_path_factory.mktemp("stem_plan") / "libstem_plan.so"
    subprocess.run([gxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-shared", "-fPIC",
                    str(REPO / "native" / "tests" / "stem_plan_capi.cpp"), "-o", str(so)], check=True)
    return ctypes.CDLL(str(so))


def _plan(lib, n, ph, cus, forced):
    out = (ctypes.c_int * 4)()
    lib.stem_band_plan_c(n, ph, cus, forced, out)
    return dict(zip(("rows", "per_image", "nbands", "grid"), out))


def _bands(lib, n, ph, cus, forced):
    nb = lib.stem_bands_c(n, ph, cus, forced, None)
    out = (ctypes.c_int * (3 * nb))()
    assert lib.stem_bands_c(n, ph, cus, forced, out) == nb
    return [tuple(out[3 * b:3 * b + 3]) for b in range(nb)]


@pytest.mark.parametrize("cus", CUS)
@pytest.mark.parametrize("ph", PHS)
def test_bands_tile_every_image(lib, ph, cus):
    for n in NS:
        for forced in (0, 1, 2, 3, ph, ph + 1):
            p = _plan(lib, n, ph, cus, forced)
            bands = _bands(lib, n, ph, cus, forced)
            where = (n, ph, cus, forced, p)
            assert p["nbands"] == len(bands) == n * p["per_image"] and p["nbands"] >= n, where
            assert 1 <= p["grid"] <= cus and p["grid"] == min(cus, p["nbands"]), where
            seen = [[0] * ph for _ in range(n)]
            for img, p0, p1 in bands:
                assert 0 <= img < n and 0 <= p0 < p1 <= ph, where  # inside one image, not empty
                assert p1 - p0 <= p["rows"], where
                for pi in range(p0, p1):
                    seen[img][pi] += 1
            assert all(c == 1 for row in seen for c in row), where  # every (n, pi) in exactly one band
            if forced:
                assert p["rows"] == min(forced, ph), where
            # the single-band query the kernel makes agrees with the list
            one = (ctypes.c_int * 3)()
            for b in (0, len(bands) // 2, len(bands) - 1):
                lib.stem_band_c(n, ph, cus, forced, b, one)
                assert tuple(one) == bands[b], where


def test_forced_one_is_one_pooled_row_per_band(lib):
    bands = _bands(lib, 3, 5, 256, 1)
    assert bands == [(n, pi, pi + 1) for n in range(3) for pi in range(5)]


def test_flagship_runs_in_one_wave(lib):
    """N = 50, PH = 87 on 256 CUs: every workgroup walks exactly one band, and few CUs stay idle."""
    p = _plan(lib, 50, 87, 256, 0)
    assert p["grid"] == p["nbands"] and 240 <= p["grid"] <= 256, p
    bands = _bands(lib, 50, 87, 256, 0)
    assert sorted(p1 - p0 for n, p0, p1 in bands if n == 0) == [15, 18, 18, 18, 18]


def test_no_plan_for_bad_arguments(lib):
    for args in [(0, 5, 256, 0), (1, 0, 256, 0), (1, 5, 0, 0), (1, 5, 256, -1), (1 << 30, 87, 256, 1)]:
        assert _plan(lib, *args)["nbands"] == 0, args
