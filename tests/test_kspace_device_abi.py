"""No GPU needed: the device-resident k-space force entries exist in every layer -- the header declares them,
the built library exports them, capi binds them and FixConp has the two methods."""
import ctypes as C
import os
import re

from conp_amd import FixConp, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("conp_ewald_compute_forces_device", "conp_pppm_compute_forces_device", "conp_debug_set_ew_block")


def test_header_declares_the_entries():
    with open(os.path.join(ROOT, "include", "conp_hip.h")) as fh:
        text = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    for name in NEW[:2]:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*)\)\s*;", text)
        assert m, name
        assert [a.split()[-1].lstrip("*") for a in m.group(1).split(",")] == ["fix", "d_x", "d_q", "d_f", "d_ev", "d_eatom"]
    assert re.search(r"\bvoid\s+conp_debug_set_ew_block\s*\(\s*int\s+n\s*\)\s*;", text)


def test_library_exports_and_capi_binds_them():
    lib = capi.load_library()
    for name in NEW:
        assert name in capi.SYMBOLS
        assert hasattr(lib, name), name
    vp = C.c_void_p
    assert lib.conp_ewald_compute_forces_device.argtypes == [vp] * 6
    assert lib.conp_pppm_compute_forces_device.argtypes == [vp] * 6
    assert lib.conp_debug_set_ew_block.argtypes == [C.c_int] and lib.conp_debug_set_ew_block.restype is None
    assert callable(FixConp.ewald_forces_device) and callable(FixConp.pppm_forces_device)
    # the hook is process-wide state on the host side only: setting and clearing it needs no device
    capi.set_ew_block(100)
    capi.set_ew_block(0)
