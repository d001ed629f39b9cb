"""no GPU: the four entries of DESIGN.md section 24 are declared with the documented parameter names, exported, listed in capi.SYMBOLS
and bound on FixConp; the two structs have the documented fields in header order; the ABI version stays 1; a NULL handle is refused."""
import ctypes as C
import os
import re

from conp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "conp_efield_set_params": ["fix", "p"],
    "conp_efield_post_force_device": ["fix", "d_x", "d_q", "d_image", "d_f", "e", "couple", "couple_scale", "d_out", "d_vatom"],
    "conp_observe_set_params": ["fix", "p"],
    "conp_observe_device": ["fix", "d_x", "d_q", "d_v", "d_image", "d_out"],
}
FIELDS = {
    "conp_efield_params": ["nlocal", "sel", "qe2f", "prd"],
    "conp_observe_params": ["nlocal", "ntypes", "ngroups", "type", "mask", "mass", "prd"],
}


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
    for struct, fields in FIELDS.items():
        assert [f for f, _ in getattr(capi, struct)._fields_] == fields
        # the struct as the header declares it, field by field and in that order
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = [n for decl in body.split(";") if decl.strip()
                    for n in re.findall(r"\*?(\w+)(?:\[\d+\])?\s*(?:,|$)", re.sub(r"^\s*(const\s+)?(int|double)\s+", "", decl.strip()))]
        assert declared == fields, struct
        assert getattr(capi, struct).prd.size == 3 * C.sizeof(C.c_double)
    assert re.search(r"#define CONP_OBSERVE_MAX_GROUPS 16\b", hdr) and re.search(r"#define CONP_OBSERVE_W 10\b", hdr)
    assert (capi.OBSERVE_MAX_GROUPS, capi.OBSERVE_W) == (16, 10)
    for src in ("conp_fieldstyle.cpp", "conp_efield.hip"):
        assert "getenv" not in open(os.path.join(ROOT, "lammps-user-conp2_amd", "csrc", src)).read()


def test_abi_version_and_null_handle():
    lib = capi.load_library()
    assert lib.conp_abi_version() == 1
    assert re.search(r"#define CONP_ABI_VERSION 1\b", open(os.path.join(ROOT, "include", "conp_hip.h")).read())
    e = (C.c_double * 3)(0.0, 0.0, 0.0)
    assert lib.conp_efield_set_params(None, C.byref(capi.conp_efield_params())) == -1
    assert lib.conp_efield_post_force_device(None, None, None, None, None, e, 0, 0.0, None, None) == -1
    assert lib.conp_observe_set_params(None, C.byref(capi.conp_observe_params())) == -1
    assert lib.conp_observe_device(None, None, None, None, None, None) == -1
