"""no GPU: the four dihedral entries are declared with the documented parameter names, exported, listed in capi.SYMBOLS and bound on
FixConp; the ABI version stays 1; a NULL handle is refused; the header states the cap on n."""
import ctypes as C
import os
import re

from conp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "conp_dihedral_set_params": ["fix", "p"],
    "conp_dihedral_set_lists": ["fix", "l"],
    "conp_dihedral_compute": ["fix", "atoms", "f", "eng", "virial", "eatom", "vatom"],
    "conp_dihedral_compute_device": ["fix", "d_x", "d_f", "d_ev", "d_eatom", "d_vatom"],
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
    for struct, fields in (("conp_dihedral_params", ["dihedral_style", "ndihedraltypes", "dihedral_coef", "improper_style", "nimpropertypes",
                                                     "improper_coef", "newton_bond"]),
                           ("conp_dihedral_lists", ["nlocal", "nall", "ndihedral", "dihedral", "nimproper", "improper", "prd"])):
        assert re.search(rf"\}} {struct};", hdr) and [f for f, _ in getattr(capi, struct)._fields_] == fields
    # the entries sit behind the bonded block, and the cap on dihedral harmonic's n is stated
    assert hdr.index("int conp_bonded_compute_device") < hdr.index("} conp_dihedral_params;") < hdr.index("int conp_integrate_set_params")
    assert re.search(r"#define CONP_DIHEDRAL_MAX_N (\d+)\b", hdr).group(1) == "12"
    assert capi.FixConp.DIHEDRAL_STYLES["opls"] == 1 and capi.FixConp.DIHEDRAL_STYLES["harmonic"] == 2
    assert capi.FixConp.IMPROPER_STYLES["harmonic"] == 1 and capi.FixConp.IMPROPER_STYLES["cvff"] == 2


def test_abi_version_and_null_handle():
    lib = capi.load_library()
    assert lib.conp_abi_version() == 1
    assert re.search(r"#define CONP_ABI_VERSION 1\b", open(os.path.join(ROOT, "include", "conp_hip.h")).read())
    p, l, at = capi.conp_dihedral_params(), capi.conp_dihedral_lists(), capi.conp_atoms()
    assert lib.conp_dihedral_set_params(None, C.byref(p)) == -1
    assert lib.conp_dihedral_set_lists(None, C.byref(l)) == -1
    assert lib.conp_dihedral_compute(None, C.byref(at), None, None, None, None, None) == -1
    assert lib.conp_dihedral_compute_device(None, None, None, None, None, None) == -1
