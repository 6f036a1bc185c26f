"""The host units of libzvx (csrc/host_*.hip, csrc/zvx.hip behind csrc/zvx_host.h) hold host code only, and the C-ABI lives where it is
said to live (no GPU needed).

The split of the host code rests on one fact: no host unit defines a kernel, so hipcc reports no kernel resources for any of them and the
device code of libzvx.so comes from the kernel units alone.  A kernel that creeps into a host unit fails here."""
import ctypes
import json
import os

import pytest

from zerovox_amd import _lib
from zerovox_amd import build as zbuild


@pytest.fixture(scope="module")
def built():
    return zbuild.build(verbose=False)


def test_host_units_define_no_kernel(built):
    # the C-ABI's two units are host units, and every host unit is built into the library
    assert {"zvx.hip", "host_comm.hip"} < set(zbuild.HOST_SOURCES)
    assert {src[:-4] for src in zbuild.HOST_SOURCES} <= {stem for stem, _src, _defs in zbuild.UNITS}
    for src in zbuild.HOST_SOURCES:
        f = os.path.join(zbuild.CSRC, src[:-4] + ".resources.json")
        assert json.load(open(f)) == {}, f"{src} defines a kernel: hipcc reported kernel resources for a host unit"
    assert zbuild.resources(), "no kernel resources recorded for the kernel units"


def test_every_bound_entry_point_is_exported(built):
    lib = ctypes.CDLL(built)
    missing = [name for name in _lib.EXPORTS if not hasattr(lib, name)]
    assert not missing, missing


def test_the_c_abi_is_in_zvx_hip_and_the_comm_unit(built):
    """Every `extern "C"` entry point is in zvx.hip, except the zvx_comm_* block: host_comm.hip keeps it, the one unit that sees RCCL's
    header.  No other host unit opens an `extern "C"`."""
    text = {src: open(os.path.join(zbuild.CSRC, src)).read() for src in zbuild.HOST_SOURCES}
    assert 'extern "C"' in text["zvx.hip"]
    assert 'extern "C"' in text["host_comm.hip"] and "zvx_comm_" in text["host_comm.hip"]
    others = [src for src in zbuild.HOST_SOURCES if src not in ("zvx.hip", "host_comm.hip")]
    assert others and all(src.startswith("host_") for src in others)
    assert [src for src in others if 'extern "C"' in text[src]] == []
