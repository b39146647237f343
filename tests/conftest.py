import os
import shutil
import sys
import tempfile
from pathlib import Path

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu)")
    config.addinivalue_line("markers", "slow: long-running test")


@pytest.fixture
def sock_dir():
    """Factory of short directories for unix sockets.  sun_path holds 107
    bytes, and pytest's tmp_path under a deep TMPDIR does not fit."""
    made = []

    def make(name="dp"):
        base = tempfile.gettempdir()
        if len(base) > 40:
            base = "/tmp"
        made.append(tempfile.mkdtemp(prefix=f"vgpu-{name}-", dir=base))
        return Path(made[-1])
    yield make
    for d in made:
        shutil.rmtree(d, ignore_errors=True)


@pytest.fixture(scope="session")
def native_build():
    """Build the native artefacts once per session (CPU: shim + fakes)."""
    from vgpu.native import build
    return build.build_all(kernels=False)


@pytest.fixture(scope="session")
def gpu_build():
    from vgpu.native import build
    return build.build_all(kernels=True)
