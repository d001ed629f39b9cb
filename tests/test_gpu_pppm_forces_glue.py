"""-m gpu: `kspace_style pppm/conp/hip ACCURACY device` (lammps_glue/pppm_conp_hip.*) executed: glue_driver's `pppmforce` mode runs
FixConpHip's hooks with the `pppm` keyword on the dilute deck, PPPMConpHip in device mode as force->kspace, and calls its
compute(eflag, vflag) on every step after the fix's pre_force, on atom->x / q / f.  Forces, per-atom energies, energy and virial
against the numpy mesh reference (tests/pppm_force_ref.py) with the bounds of tests/test_gpu_pppm_forces.py, also on a step without
a charge update (Nevery = 2); without `device` the style is what it was; the per-atom virial, `diff ad` and a missing handle stop."""
import numpy as np
import pytest

import pppm_force_ref as ref
from conp_amd import neighbor, systems
from conp_amd.capi import fix_command_for
from test_gpu_ewald_forces_glue import _kspace_output
from test_gpu_glue import run_driver, write_case

pytestmark = pytest.mark.gpu
MESH, ORDER = (27, 24, 144), 5


def _case(tmp_path, steps_of, nevery=None):
    s = systems.deck("dilute", "ffield")
    at, alist, blist = neighbor.build_lists(s)
    tokens = fix_command_for(s, extra=["pppm"])
    if nevery:
        tokens[3] = str(nevery)
    case = str(tmp_path / "case.txt")
    write_case(case, s, at, [alist, blist], tokens, steps_of(s, at), mesh=(*MESH, ORDER))
    return s, at, case


def _check_step(tag, oracle, s, at, x, res, out, step):
    n = at.nlocal
    kf, kea, ke, kv = out[step]
    assert len(kf) == n and len(kea) == n
    at2 = neighbor.Atoms(nlocal=at.nlocal, nghost=at.nghost, x=x, q=at.q.copy(), type=at.type, tag=at.tag, echeck=at.echeck, owner=at.owner)
    for i in np.nonzero(at.echeck[:n] != 0)[0]:
        at2.q[i] = res["q"][step][int(at.tag[i])]
    f, E, W, e, scale, T = ref.reference(oracle, s, at2, MESH, ORDER)
    gf = np.array([kf[int(t)] for t in at.tag[:n]])
    ge = np.array([kea[int(t)] for t in at.tag[:n]])
    for name, got, want, bound in (("force", gf, f, 1e-10 * np.abs(f).max()), ("energy", ke, E, 1e-11 * scale),
                                   ("virial", kv, W, 1e-11 * scale), ("eatom", ge, e, 1e-11 * scale)):
        err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
        print(f"{tag} {name}: max error {err:.3e}, bound {bound:.3e}")
        assert err <= bound, (tag, name, err, bound)
    return gf


def test_device_compute_matches_the_reference_also_without_a_charge_update(tmp_path, oracle):
    """`fix ... conp/hip 2 ... pppm`: on step 1 the fix's pre_force returns before b_cal, the electrolyte has moved and Verlet calls
    force->kspace->compute all the same: the result is that of the atoms at their NEW positions with the charges of step 0"""
    x1 = {}

    def steps(s, at):
        sol = at.echeck == 0
        x1["x"] = at.x.copy()
        x1["x"][sol] += np.random.default_rng(5).normal(scale=0.05, size=(int(sol.sum()), 3))
        return [(0, s.potdiff, 0, None), (1, s.potdiff, 0, x1["x"])]
    s, at, case = _case(tmp_path, steps, nevery=2)
    res, proc = run_driver(case, str(tmp_path), "pppmforce")
    assert res["rc"] == 0 and res["error"] is None, proc.stdout[-2000:] + proc.stderr[-2000:]
    out = _kspace_output(res)
    assert sorted(out) == [0, 1]
    assert res["q"][1] == res["q"][0]                    # no update on step 1
    f0 = _check_step("step 0", oracle, s, at, at.x, res, out, 0)
    f1 = _check_step("step 1 (no update, moved atoms)", oracle, s, at, x1["x"], res, out, 1)
    assert np.abs(f1 - f0).max() > 1e-3 * np.abs(f0).max()      # the atoms did move


def test_without_the_word_device_the_style_is_what_it_was(tmp_path):
    """`kspace_style pppm/conp/hip ACC` parsed by settings(): the provider mode's output, line for line (the spread's atomic adds
    arrive in no fixed order, so numbers are compared as tests/test_gpu_glue.py compares them: 1e-12)"""
    s, at, case = _case(tmp_path, lambda s, at: [(0, s.potdiff, 0, None)])
    a, pa = run_driver(case, str(tmp_path), "provider")
    b, pb = run_driver(case, str(tmp_path), "pppmhost")
    assert a["rc"] == 0 and b["rc"] == 0, pa.stdout[-2000:] + pb.stdout[-2000:] + pb.stderr[-2000:]
    la, lb = pa.stdout.split("\n"), pb.stdout.split("\n")
    assert len(la) == len(lb) and len(la) > 100
    rho_calls = [l for l in lb if l.startswith("rho_calls")]
    assert rho_calls and rho_calls == [l for l in la if l.startswith("rho_calls")]
    for x, y in zip(la, lb):
        tx, ty = x.split(), y.split()
        assert len(tx) == len(ty) and tx[:1] == ty[:1]
        for u, v in zip(tx[1:], ty[1:]):
            if u != v:
                assert float(v) == pytest.approx(float(u), rel=1e-9, abs=1e-12), (x, y)


@pytest.mark.parametrize("variant,message", [("vatom", "per-atom virial"), ("ad", "diff ik only"), ("nohandle", "needs a fix with the pppm keyword")])
def test_unsupported_requests_stop_with_their_message(tmp_path, variant, message):
    s, at, case = _case(tmp_path, lambda s, at: [(0, s.potdiff, 0, None)])
    res, proc = run_driver(case, str(tmp_path), "pppmforce", variant)
    assert res["rc"] == 2 and message in (res["error"] or ""), proc.stdout[-2000:] + proc.stderr[-2000:]
