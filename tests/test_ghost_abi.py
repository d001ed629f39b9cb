"""no GPU needed: include/conp_hip.h declares the six ghost entries of DESIGN.md section 18, the built library exports them,
capi.SYMBOLS lists them and the ABI version is still 1."""
import os
import re

from conp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["conp_ghost_build_device", "conp_ghost_fill_device", "conp_ghost_fill_int_device", "conp_ghost_fold_device", "conp_ghost_get",
           "conp_atoms_wrap_device"]


def test_the_ghost_entries_are_declared_exported_and_listed():
    hdr = open(os.path.join(ROOT, "include", "conp_hip.h")).read()
    declared = set(re.findall(r"^int\s+(conp_[a-z_0-9]+)\s*\(", hdr, re.M))
    lib = capi.load_library()
    for name in ENTRIES:
        assert name in declared, name
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS, name
    assert "conp_ghost_build_args" in hdr and re.search(r"#define CONP_ABI_VERSION 1\b", hdr)
    assert lib.conp_abi_version() == 1
    a = capi.conp_ghost_build_args()
    assert capi.C.sizeof(a) == 4 + 4 + 24 + 24 + 12 + 4 + 8          # int, (pad), 2 x double[3], int[3], (pad), double: the C layout


def test_null_handle_is_refused_without_a_device():
    lib = capi.load_library()
    assert lib.conp_ghost_fill_device(None, None, None) == -1
    assert lib.conp_ghost_fold_device(None, None, 3) == -1
    assert lib.conp_ghost_get(None, None, None, None, None) == -1
