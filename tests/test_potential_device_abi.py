"""no GPU: conp_potential_atom_device is declared with the documented parameter names, listed in
capi.SYMBOLS, bound on FixConp and -- when a built library is present -- exported and refusing NULL arguments; the ABI version stays
1; capi.potential_selection makes the flags and targets of the header from the host entry's sel / etasel; the new sources read no
environment variable and are in the Makefile."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "conp_potential_atom_device"
PARAMS = ["fix", "d_x", "d_q", "d_flags", "ntargets", "d_targets", "args", "reuse_kspace", "d_pot"]


def _library():
    return capi.load_library() if os.path.exists(capi.library_path()) else None


def test_declared_listed_bound_and_exported():
    hdr = open(os.path.join(ROOT, "include", "conp_hip.h")).read()
    m = re.search(rf"^int {NAME}\s*\((.*?)\);", hdr, re.M | re.S)
    assert m
    args = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S).split(",")
    assert [re.search(r"(\w+)\s*$", a.strip()).group(1) for a in args] == PARAMS
    assert "const conp_potential_args *args" in re.sub(r"\s+", " ", m.group(1))
    assert hdr.index("} conp_potential_args;") < m.start()          # the existing struct, declared before its second user
    assert NAME in capi.SYMBOLS and len(set(capi.SYMBOLS)) == len(capi.SYMBOLS)
    assert callable(capi.FixConp.potential_atom_device) and callable(capi.potential_selection)
    assert re.search(r"#define CONP_ABI_VERSION 1\b", hdr)
    csrc = os.path.join(ROOT, "lammps-user-conp2_amd", "csrc")
    mk = open(os.path.join(csrc, "Makefile")).read()
    for src in ("conp_potatom.hip", "conp_potatomstyle.cpp", "conp_potatomstyle.hpp"):
        assert "getenv" not in open(os.path.join(csrc, src)).read()
        assert (src if src.endswith(".hpp") else os.path.splitext(src)[0]) in mk
    assert "atomicAdd" not in open(os.path.join(csrc, "conp_potatom.hip")).read()
    lib = _library()
    if lib is None:
        return
    assert hasattr(lib, NAME) and lib.conp_abi_version() == 1
    pa = capi.conp_potential_args(pairflag=1, kspaceflag=1, qsumflag=1, eta=0.0)
    assert lib.conp_potential_atom_device(None, None, None, None, 0, None, C.byref(pa), 0, None) == -1      # CONP_ERR_ARG


def test_the_selection_helper():
    sel = np.array([0, 5, 0, 1, 1, 0, 2, 1], np.int64)               # any nonzero value selects (mask & groupbit)
    eta = np.array([1, 0, 0, 8, 0, 0, 0, 1], np.int32)
    flags, targets, nt = capi.potential_selection(sel, eta, nlocal=5)
    assert flags.dtype == np.int32 and targets.dtype == np.int32 and flags.flags.c_contiguous
    assert flags.tolist() == [2, 1, 0, 3, 1, 0, 1, 3]                # bit 0 selected, bit 1 eta_check, ghost rows included
    assert nt == 3 and targets.tolist() == [1, 3, 4]                 # the selected OWNED rows, ascending
    flags, targets, nt = capi.potential_selection(sel, None, nlocal=8)
    assert flags.tolist() == [0, 1, 0, 1, 1, 0, 1, 1] and targets.tolist() == [1, 3, 4, 6, 7] and nt == 5
    flags, targets, nt = capi.potential_selection(np.zeros(4), None, nlocal=3)
    assert nt == 0 and targets.size == 1 and not flags.any()         # an array to upload even when nobody is selected
    flags, targets, nt = capi.potential_selection(np.ones(4), None, nlocal=0)
    assert nt == 0 and flags.tolist() == [1, 1, 1, 1]
    with pytest.raises(ValueError):
        capi.potential_selection(np.ones(4), np.ones(3), nlocal=2)
    with pytest.raises(ValueError):
        capi.potential_selection(np.ones(4), None, nlocal=5)
