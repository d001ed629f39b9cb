"""no GPU needed: include/conp_hip.h declares conp_fix_post_force_device with its five parameters, the built
library exports it, capi.SYMBOLS lists it, FixConp binds it, and the ABI version is still 1."""
import inspect
import os
import re

from conp_amd import FixConp, capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "conp_fix_post_force_device"


def test_the_entry_is_declared_exported_listed_and_bound():
    hdr = open(os.path.join(ROOT, "include", "conp_hip.h")).read()
    m = re.search(r"^int\s+" + NAME + r"\s*\(([^;]*)\)\s*;", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), re.M)
    assert m, "not declared"
    params = m.group(1).split(",")
    assert [p.split()[-1].lstrip("*") for p in params] == ["fix", "d_x", "d_q", "d_f", "d_out"]
    assert ["const" in p for p in params] == [False, True, True, False, False]
    lib = capi.load_library()
    assert hasattr(lib, NAME) and NAME in capi.SYMBOLS
    assert len(getattr(lib, NAME).argtypes) == 5
    sig = inspect.signature(FixConp.post_force_device)
    assert list(sig.parameters) == ["self", "d_x", "d_q", "d_f", "d_out"]
    assert sig.parameters["d_f"].default == 0 and sig.parameters["d_out"].default == 0
    assert re.search(r"#define CONP_ABI_VERSION 1\b", hdr) and lib.conp_abi_version() == 1


def test_null_handle_is_refused_without_a_device():
    lib = capi.load_library()
    assert getattr(lib, NAME)(None, None, None, None, None) == -1
