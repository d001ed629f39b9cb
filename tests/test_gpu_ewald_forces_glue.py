"""-m gpu: `kspace_style ewald/conp/hip` (lammps_glue/ewald_conp_hip.*) executed: glue_driver's `kspace` mode runs FixConpHip's hooks on
the dilute deck with EwaldConpHip as force->kspace and calls its compute(eflag, vflag) on every step after the fix's pre_force, on
atom->x / q / f; it prints forces, per-atom energies, energy and virial per step.  The same library through ctypes
(FixConp.ewald_forces) gives the same numbers to 1e-12; on a step without a charge update (Nevery = 2) the style still follows the
atoms; without an Ewald parameter it stops."""
import dataclasses

import numpy as np
import pytest

import ewald_force_ref as ref
from conp_amd import FixConp, neighbor, systems
from conp_amd.capi import fix_command_for
from test_gpu_glue import run_driver, write_case

pytestmark = pytest.mark.gpu


def _kspace_output(res):
    """{step: (forces by tag, eatom by tag, energy, virial)} of the driver's `kspace` mode"""
    steps = {}
    for line in res["screen"]:
        t = line.split()
        if t and t[0] in ("kf", "kea", "ke", "kv"):
            kf, kea, sc = steps.setdefault(int(t[1]), ({}, {}, {}))
            if t[0] == "kf":
                kf[int(t[2])] = [float(v) for v in t[3:6]]
            elif t[0] == "kea":
                kea[int(t[2])] = float(t[3])
            elif t[0] == "ke":
                sc["ke"] = float(t[2])
            else:
                sc["kv"] = np.array([float(v) for v in t[2:8]])
    return {ts: (kf, kea, sc["ke"], sc["kv"]) for ts, (kf, kea, sc) in steps.items()}


def test_kspace_style_compute_matches_the_ctypes_path(tmp_path):
    s = systems.deck("dilute", "ffield")
    at, alist, blist = neighbor.build_lists(s)
    lists = [alist] if alist is blist else [alist, blist]
    case = str(tmp_path / "case.txt")
    write_case(case, s, at, lists, fix_command_for(s), [(0, s.potdiff, 0, None)])
    res, proc = run_driver(case, str(tmp_path), "kspace")
    assert res["rc"] == 0 and res["error"] is None, proc.stdout[-2000:] + proc.stderr[-2000:]
    kf, kea, ke, kv = _kspace_output(res)[0]
    n = at.nlocal
    assert len(kf) == n and len(kea) == n

    fx = FixConp(s)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)
    f, E, W, e = fx.ewald_forces(at, eatom=True)
    fx.close()
    gf = np.array([kf[int(t)] for t in at.tag[:n]])
    ge = np.array([kea[int(t)] for t in at.tag[:n]])
    assert np.abs(f).max() > 0
    assert np.abs(gf - f).max() <= 1e-12 * np.abs(f).max()
    assert np.abs(ge - e).max() <= 1e-12 * np.abs(e).max()
    assert abs(ke - E) <= 1e-12 * abs(E)
    assert np.abs(kv - W).max() <= 1e-12 * np.abs(W).max()


def test_kspace_style_follows_the_atoms_on_steps_without_a_charge_update(tmp_path):
    """`fix ... conp/hip 2`: on step 1 the fix's pre_force returns before b_cal, the electrolyte has moved, and Verlet calls
    force->kspace->compute all the same.  The style must form S of the atoms it is given, not contract the S of step 0 with the
    phases of step 1: forces, energy and virial of step 1 against the numpy reference (tests/ewald_force_ref.py) at the NEW
    positions and the charges of step 0, with the bounds of tests/test_gpu_ewald_forces.py (1e-10 max|f|; 1e-11 of the unsubtracted
    scale)."""
    s = systems.deck("dilute", "ffield")
    at, alist, blist = neighbor.build_lists(s)
    lists = [alist] if alist is blist else [alist, blist]
    n = at.nlocal
    sol = at.echeck == 0
    x1 = at.x.copy()
    x1[sol] += np.random.default_rng(5).normal(scale=0.05, size=(int(sol.sum()), 3))
    tokens = fix_command_for(s)
    tokens[3] = "2"                                      # Nevery
    case = str(tmp_path / "case.txt")
    write_case(case, s, at, lists, tokens, [(0, s.potdiff, 0, None), (1, s.potdiff, 0, x1)])
    res, proc = run_driver(case, str(tmp_path), "kspace")
    assert res["rc"] == 0 and res["error"] is None, proc.stdout[-2000:] + proc.stderr[-2000:]
    out = _kspace_output(res)
    assert sorted(out) == [0, 1]
    assert res["q"][1] == res["q"][0]                    # no update on step 1
    q = at.q[:n].copy()
    for i in np.nonzero(at.echeck[:n] != 0)[0]:
        q[i] = res["q"][1][int(at.tag[i])]

    fx = FixConp(s)                                      # (only for the library's k list and ug)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    T = ref.handle_tables(fx, s)
    fx.close()
    x = np.ascontiguousarray(x1[:n])
    S = ref.structure_factor(x, q, T["kv"])
    E, W = ref.energy_virial(S, x, q, T["kv"], T["ug"], T["g"], T["V"], T["qs"], T["slab"], T["L"])
    f, e = ref.forces_eatom(S, x, q, T["kv"], T["ug"], T["g"], T["V"], T["qs"], np.arange(n), T["slab"], T["L"])
    scale = T["qs"] * ref.ksum(S, T["ug"])
    kf, kea, ke, kv = out[1]
    gf = np.array([kf[int(t)] for t in at.tag[:n]])
    ge = np.array([kea[int(t)] for t in at.tag[:n]])
    f0 = np.array([out[0][0][int(t)] for t in at.tag[:n]])
    assert np.abs(gf - f0).max() > 1e-3 * np.abs(f0).max()      # the atoms did move
    for name, got, want, bound in (("force", gf, f, 1e-10 * np.abs(f).max()), ("energy", ke, E, 1e-11 * scale),
                                   ("virial", kv, W, 1e-11 * scale), ("eatom", ge, e, 1e-11 * scale)):
        err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
        print(f"step 1 {name}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (name, err, bound)


def test_kspace_style_stops_without_an_ewald_parameter(tmp_path):
    """the style does not estimate g_ewald from the accuracy: without `kspace_modify gewald` init() stops, before the fix reads 0"""
    s = dataclasses.replace(systems.deck("dilute", "ffield"), g_ewald=0.0)
    at, alist, blist = neighbor.build_lists(s)
    lists = [alist] if alist is blist else [alist, blist]
    case = str(tmp_path / "case.txt")
    write_case(case, s, at, lists, fix_command_for(s), [(0, s.potdiff, 0, None)])
    res, proc = run_driver(case, str(tmp_path), "kspace")
    assert res["rc"] == 2 and "kspace_modify gewald" in (res["error"] or ""), proc.stdout[-2000:] + proc.stderr[-2000:]
