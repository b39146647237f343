"""The kernels' shared helpers have one definition each, in a header.

pack2 and f2bf are the rounding that the bit-exact GPU suites hold every
kernel to, and the activation codes are a contract between Python and the
kernel files; a private copy in one .hip file could drift unnoticed.  This
reads native/kernels as text (no compiler, no GPU)."""
import re
from pathlib import Path

import pytest

KERNELS = Path(__file__).resolve().parents[1] / "native" / "kernels"
SOURCES = sorted(KERNELS.glob("*.hip")) + sorted(KERNELS.glob("*.h"))
HELPERS = ("unpack8", "pack2", "pack8", "bf2f", "f2bf", "load8f", "store8f", "wave_sum", "act_fwd", "act_grad")


def _defining_files(name: str) -> list[str]:
    """Files with `__forceinline__ <return type> name(`: a definition, not a call."""
    pat = re.compile(r"__forceinline__\s+[\w:<>\s\*&]*?\b" + name + r"\s*\(")
    return [p.name for p in SOURCES if pat.search(p.read_text())]


def test_sources_found():
    assert len([p for p in SOURCES if p.suffix == ".hip"]) >= 17


@pytest.mark.parametrize("name", HELPERS)
def test_helper_defined_in_one_header(name):
    files = _defining_files(name)
    assert len(files) == 1 and files[0].endswith(".h"), f"{name} is defined in {files}"


def test_export_macro_defined_once():
    files = [p.name for p in SOURCES for _ in re.findall(r"^\s*#\s*define\s+VGPU_API\b", p.read_text(), re.M)]
    assert files == ["bf16.h"], files
