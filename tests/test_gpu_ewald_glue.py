"""-m gpu: the Ewald per-atom potentials through the LAMMPS glue, EXECUTED by glue_driver: KSpaceModuleHip's
compute_group_potential / compute_particle_potential (the reference's KSpaceModuleEwald leaves them at `return 0.`,
kspacemodule.h:38-39), and `compute potential/atom/hip` without a pppm style -- its setup() takes the handle of the reference's
fix conp with the KSpaceModuleHip provider, or of a conp/hip fix.  Equal to the ctypes calls of the same library on the same atoms."""
import numpy as np
import pytest

from conp_amd import FixConp, neighbor, systems
from conp_amd.capi import fix_command_for
from test_gpu_glue import run_driver, write_case

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("mode", ["slab", "ffield"])
def test_ewald_provider_potentials_executed(tmp_path, mode):
    s = systems.small_random(ne_side=4, n_elyte=96, lz=60.0, mode=mode)
    at, alist, blist = neighbor.build_lists(s)
    case = str(tmp_path / "case.txt")
    write_case(case, s, at, [alist] if alist is blist else [alist, blist], fix_command_for(s), [(0, s.potdiff, 0, None)])
    res, proc = run_driver(case, str(tmp_path), "provider")
    assert res["rc"] == 0 and res["error"] is None, proc.stdout[-2000:] + proc.stderr[-2000:]
    u, up, cp = {}, {}, {}
    for line in proc.stdout.splitlines():
        t = line.split()
        if t and t[0] in ("u", "up", "cp"):
            {"u": u, "up": up, "cp": cp}[t[0]][int(t[1])] = float(t[2])
    fx = FixConp(s)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    n = at.nlocal
    fx.km_conp_setup(float((at.q[:n] ** 2).sum()), n)         # the provider's k tables (km_ewald.cpp:63-132)
    tags = at.tag[:n]
    sel = (at.echeck[:n] == 1).astype(np.int32)                # group 1 of the driver = eleleft
    want = fx.ewald_group_potential(at, sel)
    assert sorted(u) == sorted(int(t) for t in tags[sel != 0])
    scale = np.abs(want).max()
    for i in np.nonzero(sel)[0]:
        assert abs(u[int(tags[i])] - want[i]) <= 1e-11 * scale
    fx.ewald_compute(at)
    assert sorted(up) == sorted(int(t) for t in tags)
    for i in range(0, n, 7):
        assert abs(up[int(tags[i])] - fx.ewald_particle_potential(at, i)) <= 1e-11 * scale
    # compute potential/atom/hip kspace, found through the fix's kspmod: == conp_compute_potential_atom through ctypes
    _check_compute(cp, fx, at, alist)
    fx.close()


def _check_compute(cp, fx, at, plist):
    n = at.nlocal
    want = fx.compute_potential_atom(at, plist, np.ones(at.nlocal + at.nghost, np.int32), pair=False, kspace=True, qsum=True)[:n]
    tags = at.tag[:n]
    assert sorted(cp) == sorted(int(t) for t in tags)
    got = np.array([cp[int(t)] for t in tags])
    assert np.abs(want).max() > 0
    assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max()


@pytest.mark.parametrize("mode", ["slab", "ffield"])
def test_compute_potential_atom_on_a_conp_hip_fix_under_ewald(tmp_path, mode):
    """`fix conp/hip` with Ewald + `compute potential/atom/hip kspace`: setup() finds the fix's handle, the per-atom output (volts) equals
    the ctypes call on a handle given the same hooks"""
    s = systems.small_random(ne_side=4, n_elyte=96, lz=60.0, mode=mode)
    at, alist, blist = neighbor.build_lists(s)
    case = str(tmp_path / "case.txt")
    write_case(case, s, at, [alist] if alist is blist else [alist, blist], fix_command_for(s), [(0, s.potdiff, 0, None)])
    res, proc = run_driver(case, str(tmp_path), "compute")
    assert res["rc"] == 0 and res["error"] is None, proc.stdout[-2000:] + proc.stderr[-2000:]
    cp = {}
    for line in proc.stdout.splitlines():
        t = line.split()
        if t and t[0] == "cp":
            cp[int(t[1])] = float(t[2])
    fx = FixConp(s)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)                       # the charges the fix wrote before the compute ran
    _check_compute(cp, fx, at, alist)
    fx.close()
