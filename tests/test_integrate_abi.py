"""no GPU: the seven integration entries are declared with the documented parameter names, exported, listed in capi.SYMBOLS and bound
on FixConp; the struct has the documented fields; the ABI version stays 1; a NULL handle is refused."""
import ctypes as C
import os
import re

from conp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "conp_integrate_set_params": ["fix", "p"],
    "conp_integrate_setup_device": ["fix", "d_v", "t_target"],
    "conp_integrate_initial_device": ["fix", "d_x", "d_v", "d_f", "t_target"],
    "conp_integrate_final_device": ["fix", "d_v", "d_f", "d_out"],
    "conp_integrate_temperature_device": ["fix", "d_v", "d_out"],
    "conp_integrate_get_state": ["fix", "state"],
    "conp_integrate_set_state": ["fix", "state"],
}
FIELDS = ["nlocal", "ntypes", "ngroups", "type", "group", "mass", "style", "dof", "t_period", "dt", "ftm2v", "mvv2e", "boltz"]


def test_declared_exported_listed_and_bound():
    hdr = open(os.path.join(ROOT, "include", "conp_hip.h")).read()
    lib = capi.load_library()
    for name, params in ENTRIES.items():
        m = re.search(rf"^int {name}\s*\((.*?)\);", hdr, re.M | re.S)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
        assert [re.search(r"(\w+)\s*$", a.strip()).group(1) for a in args] == params, name
        assert hasattr(lib, name) and name in capi.SYMBOLS
        assert callable(getattr(capi.FixConp, name[len("conp_"):]))
    assert re.search(r"\} conp_integrate_params;", hdr) and [f for f, _ in capi.conp_integrate_params._fields_] == FIELDS
    # the struct as the header declares it, field by field and in that order
    body = re.search(r"typedef struct \{([^}]*)\} conp_integrate_params;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = [n for decl in body.split(";") for n in re.findall(r"\*?(\w+)\s*(?:,|$)", decl.strip()) if decl.strip()]
    assert declared == FIELDS
    assert re.search(r"#define CONP_INTEGRATE_MAX_GROUPS 8\b", hdr) and re.search(r"#define CONP_INTEGRATE_CHAIN 3\b", hdr)


def test_abi_version_and_null_handle():
    lib = capi.load_library()
    assert lib.conp_abi_version() == 1
    assert re.search(r"#define CONP_ABI_VERSION 1\b", open(os.path.join(ROOT, "include", "conp_hip.h")).read())
    p = capi.conp_integrate_params()
    t = (C.c_double * 8)()
    assert lib.conp_integrate_set_params(None, C.byref(p)) == -1
    assert lib.conp_integrate_setup_device(None, None, t) == -1
    assert lib.conp_integrate_initial_device(None, None, None, None, t) == -1
    assert lib.conp_integrate_final_device(None, None, None, None) == -1
    assert lib.conp_integrate_temperature_device(None, None, None) == -1
    assert lib.conp_integrate_get_state(None, t) == -1
    assert lib.conp_integrate_set_state(None, t) == -1
