"""-m gpu: `kspace_style ewald/conp/hip` tallies the per-atom virial (lammps_glue/ewald_conp_hip.*):
glue_driver's `kspace vatom` mode asks compute() for vflag | 4 on every step and prints one `kva STEP TAG v0..v5` line per owned atom.
They agree with the numpy reference (tests/kspace_vatom_ref.py) within 1e-11 of the unsubtracted scale, also on a step without a charge
update (Nevery = 2); without the word the mode prints no such line."""
import numpy as np
import pytest

import ewald_force_ref as ref
import kspace_vatom_ref as vref
from conp_amd import FixConp, neighbor, systems
from conp_amd.capi import fix_command_for
from test_gpu_glue import run_driver, write_case

pytestmark = pytest.mark.gpu


def _kva(res):
    out = {}
    for line in res["screen"]:
        t = line.split()
        if t and t[0] == "kva":
            out.setdefault(int(t[1]), {})[int(t[2])] = [float(v) for v in t[3:9]]
    return out


def test_kspace_style_tallies_the_per_atom_virial(tmp_path):
    s = systems.deck("dilute", "ffield")
    at, alist, blist = neighbor.build_lists(s)
    lists = [alist] if alist is blist else [alist, blist]
    n = at.nlocal
    sol = at.echeck == 0
    x1 = at.x.copy()
    x1[sol] += np.random.default_rng(5).normal(scale=0.05, size=(int(sol.sum()), 3))
    tokens = fix_command_for(s)
    tokens[3] = "2"                                      # Nevery: no charge update on step 1, the atoms have moved
    case = str(tmp_path / "case.txt")
    write_case(case, s, at, lists, tokens, [(0, s.potdiff, 0, None), (1, s.potdiff, 0, x1)])
    res, proc = run_driver(case, str(tmp_path), "kspace", "vatom")
    assert res["rc"] == 0 and res["error"] is None, proc.stdout[-2000:] + proc.stderr[-2000:]
    kva = _kva(res)
    assert sorted(kva) == [0, 1] and all(len(kva[ts]) == n for ts in kva)
    assert res["q"][1] == res["q"][0]                    # no update on step 1

    fx = FixConp(s)                                      # (only for the library's k list and ug)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    T = ref.handle_tables(fx, s)
    fx.close()
    kv_lines = {int(t.split()[1]): np.array([float(v) for v in t.split()[2:8]]) for t in res["screen"] if t.startswith("kv ")}
    for ts, xs in ((0, at.x), (1, x1)):
        q = at.q[:n].copy()
        for i in np.nonzero(at.echeck[:n] != 0)[0]:
            q[i] = res["q"][ts][int(at.tag[i])]
        x = np.ascontiguousarray(xs[:n])
        S = ref.structure_factor(x, q, T["kv"])
        want = vref.ewald_vatom(S, x, q, T["kv"], T["ug"], T["g"], T["qs"], np.arange(n))
        scale = T["qs"] * ref.ksum(S, T["ug"])
        got = np.array([kva[ts][int(t)] for t in at.tag[:n]])
        err = float(np.abs(got - want).max())
        print(f"step {ts} vatom: max error {err:.3e}, bound {1e-11 * scale:.3e} ({err / (1e-11 * scale):.3g} of it)")
        assert np.abs(want).max() > 0 and err <= 1e-11 * scale
        assert np.abs(got.sum(axis=0) - kv_lines[ts]).max() <= 1e-11 * scale      # the step's own global virial
    assert np.abs(np.array(list(kva[1].values())) - np.array(list(kva[0].values()))).max() > 0       # the atoms did move


def test_kspace_mode_without_the_word_prints_no_kva_line(tmp_path):
    s = systems.deck("dilute", "ffield")
    at, alist, blist = neighbor.build_lists(s)
    lists = [alist] if alist is blist else [alist, blist]
    case = str(tmp_path / "case.txt")
    write_case(case, s, at, lists, fix_command_for(s), [(0, s.potdiff, 0, None)])
    res, proc = run_driver(case, str(tmp_path), "kspace")
    assert res["rc"] == 0 and res["error"] is None, proc.stdout[-2000:] + proc.stderr[-2000:]
    assert not _kva(res) and any(t.startswith("kv ") for t in res["screen"])
