"""no GPU needed: conp_fix_post_neighbor_device and conp_fix_get_step_tables are declared in
include/conp_hip.h, exported by the library and listed in capi.SYMBOLS; the ABI version stays 1; without a handle both refuse."""
import os
import re

from conp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["conp_fix_post_neighbor_device", "conp_fix_get_step_tables"]


def test_header_exports_and_symbol_list_carry_the_entries():
    hdr = open(os.path.join(ROOT, "include", "conp_hip.h")).read()
    lib = capi.load_library()
    for name in ENTRIES:
        assert re.search(r"^int\s+%s\s*\(" % name, hdr, re.M), name
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS
    assert re.search(r"#define CONP_ABI_VERSION 1\b", hdr) and lib.conp_abi_version() == 1
    assert len(capi.FixConp.STEP_TABLES) == 9
    assert lib.conp_fix_post_neighbor_device(None, None, None) == -1
    assert lib.conp_fix_get_step_tables(None, None, *([None] * 9)) == -1
