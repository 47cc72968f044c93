"""CPU: the entry points that came with k_mm_reuse are declared in the header's "later, without a new number" list, exported
by libtclip.so, bound in _capi, and the mode switch refuses what it does not know - all without a GPU."""
import ctypes
import os
import re

from conftest import ROOT
from tclip_amd import _capi

NAMES = ("tclip_debug_set_mm_reuse", "tclip_profile_last_mm_reuse")


def test_reuse_entry_points_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "tclip.h")).read()
    version_comment = header[:header.index("#define TCLIP_ABI_VERSION")]
    later = version_comment[version_comment.index("later, without a new number"):]
    assert re.search(r"#define\s+TCLIP_ABI_VERSION\s+5\b", header)
    lib = _capi.lib()
    for name in NAMES:
        assert name in later, f"{name} is not in the header's list of later additions"
        assert re.search(r"\bint\s+" + name + r"\s*\(", header[header.index("#define TCLIP_ABI_VERSION"):]), f"{name} is not declared"
        assert name in _capi.EXPORTS
        assert hasattr(lib, name), f"{name} is not exported by libtclip.so"
    assert lib.tclip_abi_version() == 5


def test_reuse_mode_switch_refuses_unknown_modes():
    lib = _capi.lib()
    try:
        for bad in (3, -1):
            assert lib.tclip_debug_set_mm_reuse(bad) != 0
            assert b"tclip_debug_set_mm_reuse" in lib.tclip_last_error()
        for ok in (0, 2, 1):
            assert lib.tclip_debug_set_mm_reuse(ok) == 0
        assert lib.tclip_profile_last_mm_reuse(None) != 0 and b"null" in lib.tclip_last_error()
        out = (ctypes.c_uint64 * 2)(7, 7)
        assert lib.tclip_profile_last_mm_reuse(out) == 0 and list(out) == [0, 0]      # nothing collected in this process
    finally:
        lib.tclip_debug_set_mm_reuse(1)
