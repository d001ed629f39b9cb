"""no GPU: the five entries of DESIGN.md section 25 are declared with the documented parameter names, listed in capi.SYMBOLS, bound on
FixConp and -- when a built library is present -- exported; the three structs have the documented fields in header order; the ABI
version stays 1; a NULL handle is refused; the header's section 24 points to section 25 for fix zmirror."""
import ctypes as C
import os
import re

from conp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {
    "conp_pair_set_exclusions": ["fix", "e"],
    "conp_pair_build_list_exclude_device": ["fix", "d_x", "a", "at"],
    "conp_zmirror_set_params": ["fix", "p"],
    "conp_zmirror_post_integrate_device": ["fix", "d_x", "ntimestep"],
    "conp_zmirror_get_map": ["fix", "npairs", "src", "dst"],
}
FIELDS = {
    "conp_pair_exclusions": ["ntypes", "ntype_pairs", "type_i", "type_j", "ngroup_pairs", "group_bit1", "group_bit2", "nmol", "mol_bit",
                             "mol_intra"],
    "conp_pair_exclude_atoms": ["d_type", "d_mask", "d_molecule"],
    "conp_zmirror_params": ["nlocal", "tag", "mask", "groupbit", "jgroupbit", "nevery", "boxlo_z", "zprd"],
}


def _library():
    return capi.load_library() if os.path.exists(capi.library_path()) else None


def test_declared_listed_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "conp_hip.h")).read()
    lib = _library()
    for name, params in ENTRIES.items():
        m = re.search(rf"^int {name}\s*\((.*?)\);", hdr, re.M | re.S)
        assert m, name
        args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
        assert [re.search(r"(\w+)\s*$", a.strip()).group(1) for a in args] == params, name
        assert name in capi.SYMBOLS
        assert callable(getattr(capi.FixConp, name[len("conp_"):]))
        if lib is not None:
            assert hasattr(lib, name), name
    for struct, fields in FIELDS.items():
        assert [f for f, _ in getattr(capi, struct)._fields_] == fields
        body = re.search(r"typedef struct \{([^}]*)\} %s;" % struct, hdr).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        declared = [n for decl in body.split(";") if decl.strip()
                    for n in re.findall(r"\*?(\w+)\s*(?:,|$)", re.sub(r"^\s*(const\s+)?(int|double)\s+", "", decl.strip()))]
        assert declared == fields, struct
    assert "Out of scope: fix zmirror" not in hdr and re.search(r"fix zmirror: conp_zmirror_\* below \(DESIGN.md section 25\)", hdr)
    for src in ("conp_zmirrorstyle.cpp", "conp_zmirror.hip", "conp_neigh.hip", "conp_pairstyle.cpp"):
        assert "getenv" not in open(os.path.join(ROOT, "lammps-user-conp2_amd", "csrc", src)).read()


def test_abi_version_and_null_handle():
    assert re.search(r"#define CONP_ABI_VERSION 1\b", open(os.path.join(ROOT, "include", "conp_hip.h")).read())
    lib = _library()
    if lib is None:
        return
    assert lib.conp_abi_version() == 1
    assert lib.conp_pair_set_exclusions(None, None) == -1
    assert lib.conp_pair_build_list_exclude_device(None, None, C.byref(capi.conp_pair_build_args()), C.byref(capi.conp_pair_exclude_atoms())) == -1
    assert lib.conp_zmirror_set_params(None, C.byref(capi.conp_zmirror_params())) == -1
    assert lib.conp_zmirror_post_integrate_device(None, None, 0) == -1
    assert lib.conp_zmirror_get_map(None, None, None, None) == -1
