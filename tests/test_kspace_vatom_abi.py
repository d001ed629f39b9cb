"""No GPU: the four per-atom-virial entries are declared in include/conp_hip.h, exported by the built library
and bound in capi.py; INTEGRATION.md names them and the driver's new word."""
import os
import re

from conp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ["conp_ewald_compute_forces_vatom", "conp_pppm_compute_forces_vatom", "conp_ewald_compute_forces_vatom_device",
           "conp_pppm_compute_forces_vatom_device"]


def test_the_entries_are_in_the_header_the_library_and_the_binding():
    hdr = open(os.path.join(ROOT, "include", "conp_hip.h")).read()
    lib = capi.load_library()
    for name in ENTRIES:
        assert re.search(r"^int\s+" + name + r"\s*\(", hdr, re.M), name
        assert hasattr(lib, name), name
        assert name in capi.SYMBOLS, name
    for method in ("ewald_forces_vatom", "pppm_forces_vatom", "ewald_forces_vatom_device", "pppm_forces_vatom_device"):
        assert hasattr(capi.FixConp, method), method
    assert len(lib.conp_ewald_compute_forces_vatom.argtypes) == 7 and len(lib.conp_pppm_compute_forces_vatom_device.argtypes) == 7
    assert lib.conp_abi_version() == 1


def test_the_new_words_are_in_the_integration_guide():
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    for word in ENTRIES + ["stress/atom", "kspace vatom"]:
        assert word in doc, word
