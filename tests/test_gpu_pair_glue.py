"""-m gpu: `pair_style lj/cut/coul/long/conp/hip` (lammps_glue/pair_lj_cut_coul_long_conp_hip.*) executed: glue_driver's `pair` mode runs
FixConpHip's hooks on the small box with PairLJCutCoulLongConpHip as force->pair and calls its compute(eflag, vflag) on every step
after the fix's pre_force, on atom->x / q / f.  Three steps: setup, a step with a re-neighbour at moved positions, a step without.
The same library through ctypes (FixConp.pair_compute) on the same positions and the charges the driver printed: forces, eatom and
vatom to the bounds of tests/test_gpu_pair_forces.py against the reference AND against each other, `pe` / `pv` bit-equal.  The list
is uploaded at the setup and at the re-neighbour only.  A table request (pair_modify table left at 12) stops with the style's message."""
import dataclasses

import numpy as np
import pytest

import pair_force_ref as pref
from conp_amd import FixConp, neighbor, systems
from conp_amd.capi import fix_command_for
from test_gpu_glue import run_driver, write_case
from test_gpu_pair_forces import TOL, _frac, check

pytestmark = pytest.mark.gpu


def _setup(tmp_path, special=True):
    s = dataclasses.replace(systems.small_random(ne_side=4, n_elyte=64, seed=pref.SEED), eletypes=None)
    at, lst, _ = neighbor.build_lists(s, special_frac=0.2 if special else 0.0)
    p = pref.lj_tables(s.ntypes, s.cutoff)
    sl, sc = (pref.SPECIAL_LJ, pref.SPECIAL_COUL) if special else (pref.ONES, pref.ONES)
    n = at.nlocal
    rng = np.random.default_rng(17)
    img = at.x[n:] - at.x[at.owner[n:]]
    xs = [at.x.copy()]
    for _ in range(2):                                   # the electrolyte moves 0.02 A per step, the ghosts with their owners
        x = xs[-1].copy()
        sol = at.echeck[:n] == 0
        x[:n][sol] += rng.normal(scale=0.02, size=(int(sol.sum()), 3))
        x[n:] = x[at.owner[n:]] + img
        xs.append(x)
    steps = [(0, s.potdiff, 0, None), (1, s.potdiff, 1, xs[1]), (2, s.potdiff, 0, xs[2])]
    case = str(tmp_path / "case.txt")
    write_case(case, s, at, [lst], fix_command_for(s), steps)
    nt1 = s.ntypes + 1
    tabs = [p.cutsq] + [p.lj[k] for k in ("cut_ljsq", "lj1", "lj2", "lj3", "lj4", "offset")]
    with open(case, "a") as fh:                          # the optional block behind the steps, read by the pair mode only
        fh.write("pair " + repr(float(p.cut_coul)) + "\n")
        for tab in tabs:
            assert tab.shape == (nt1, nt1)
            fh.write(" ".join(repr(float(v)) for v in tab.ravel()) + "\n")
        fh.write(" ".join(repr(float(v)) for v in sl) + "\n" + " ".join(repr(float(v)) for v in sc) + "\n")
    return s, at, lst, p, sl, sc, xs, case


def _pair_output(res, nall, vatom):
    steps = {}
    for line in res["screen"]:
        t = line.split()
        if not t or t[0] not in ("pf", "pea", "pva", "pe", "pv", "pls"):
            continue
        d = steps.setdefault(int(t[1]), dict(f=np.full((nall, 3), np.nan), ea=np.full(nall, np.nan), va=np.full((nall, 6), np.nan)))
        v = [float(w) for w in t[2:]]
        if t[0] == "pf":
            d["f"][int(t[2])] = v[1:]
        elif t[0] == "pea":
            d["ea"][int(t[2])] = v[1]
        elif t[0] == "pva":
            d["va"][int(t[2])] = v[1:]
        elif t[0] == "pe":
            d["eng"] = np.array(v)
        elif t[0] == "pv":
            d["W"] = np.array(v)
        else:
            d["uploads"] = int(t[2])
    for d in steps.values():
        assert np.isfinite(d["f"]).all() and np.isfinite(d["ea"]).all() and (np.isfinite(d["va"]).all() or not vatom)
    return steps


@pytest.mark.parametrize("vatom", [False, True])
def test_pair_style_compute_matches_the_ctypes_path(tmp_path, vatom):
    s, at, lst, p, sl, sc, xs, case = _setup(tmp_path)
    res, proc = run_driver(case, str(tmp_path), "pair", *(["vatom"] if vatom else []))
    assert res["rc"] == 0 and res["error"] is None, proc.stdout[-2000:] + proc.stderr[-2000:]
    out = _pair_output(res, at.nall, vatom)
    assert sorted(out) == [0, 1, 2]
    assert [out[k]["uploads"] for k in (0, 1, 2)] == [1, 2, 2]          # the setup and the re-neighbour, not the plain step

    fx = FixConp(s)
    fx.init_lists(lst, lst)
    fx.setup_post_neighbor(at)
    fx.pair_set_params(p.cutsq, p.cut_coul, p.lj, sl, sc)
    fx.pair_set_list(lst, at.nall)
    moved = False
    for step in (0, 1, 2):
        a = dataclasses.replace(at, x=np.ascontiguousarray(xs[step]), q=at.q.copy())
        qtag = res["q"][step]                           # the electrode charges the driver's fix wrote (printed with 17 digits)
        for i in np.nonzero(a.echeck != 0)[0]:
            a.q[i] = qtag[int(a.tag[i])]
        assert np.abs(a.q[a.echeck != 0]).max() > 0
        f, eng, W, ea, va = fx.pair_compute(a)
        R = pref.for_atoms(a, lst, p, s, False, sl, sc)
        d = out[step]
        check(f"pair style, step {step}", (d["f"], d["eng"], d["W"], d["ea"], d["va"] if vatom else None), R)
        assert _frac(f"step {step}: style against ctypes, force", d["f"], f, TOL * R.A[:, None]) <= 1.0
        assert d["eng"].tobytes() == eng.tobytes() and d["W"].tobytes() == W.tobytes()        # pe / pv: fixed-order sums, same input
        if step:
            moved = moved or np.abs(d["f"] - out[0]["f"]).max() > 0
    assert moved
    fx.close()


def test_pair_style_refuses_coulomb_tables(tmp_path):
    s, at, lst, p, sl, sc, xs, case = _setup(tmp_path, special=False)
    res, proc = run_driver(case, str(tmp_path), "pair", "table")
    assert res["rc"] == 2, proc.stdout[-2000:] + proc.stderr[-2000:]
    assert "does not support Coulomb tables" in (res["error"] or "") and "pair_modify table 0" in res["error"]
