"""-m gpu: conp_pppm_compute_forces -- PPPM reciprocal-space forces, energy, virial and per-atom energies on the device (DESIGN.md
section 13): what PPPM::compute does after the charge update.

(1) against the numpy mesh reference of tests/pppm_force_ref.py (same mesh arithmetic; guarded by tests/test_pppm_force_math.py) on
    ALL owned atoms, zero-charge probes included, and against the exact Ewald sum within twice the mesh error measured for that
    reference on the CPU;  (2) accumulation into f, NULL outputs;  (3) the contract: moved atoms without an update, keep_density on
    and off, the mesh-potential cache, the Ewald handle refuses;  (4) guard zones.
Bounds: forces 1e-10 max|f|; energy, virial and per-atom energies 1e-11 of qs (V / 2) sum G |rho^|^2 / N^2, the unsubtracted scale
(those of tests/test_gpu_ewald_forces.py and the 1e-11 of the PPPM b test).
Sizes: tests/test_gpu_pppm_forces_sizes.py; ranks: tests/test_gpu_pppm_forces_ranks.py; the glue: tests/test_gpu_pppm_forces_glue.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import pppm_force_ref as ref
from conp_amd import ConpError, FixConp, neighbor, systems

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compare(tag, got, want, bound):
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    print(f"{tag}: max error {err:.3e}, bound {bound:.3e} ({err / bound:.3g} of it)")
    assert err <= bound, (tag, err, bound)


def _handle(deck, mode, mesh, order):
    s = systems.deck(deck, mode, etypes=True)
    at, alist, blist = neighbor.build_lists(s)
    fx = FixConp(s, extra_args=["pppm"], pppm_mesh=mesh, pppm_order=order)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)               # electrode atoms carry their solved charges from here on
    return s, at, alist, blist, fx


def _add_probes(s, at, n=4):
    """zero-charge probes (four electrolyte atoms made into them) near the box centre"""
    el = np.nonzero((at.echeck[:at.nlocal] == 0) & (at.q[:at.nlocal] != 0))[0][:n]
    centre = s.boxlo + 0.5 * np.asarray(s.prd)
    for k, i in enumerate(el):
        at.q[i] = 0.0
        at.x[i] = centre + np.array([0.37 * k, -0.21 * k, 0.53 * k - 0.8])
    return el


def check_against_reference(tag, oracle, s, at, fx, mesh, order, targets=None, probes=()):
    """one call with every output, against the numpy mesh reference; returns (got, want) tuples"""
    n = at.nlocal
    f, E, W, e, scale, T = ref.reference(oracle, s, at, mesh, order, targets)
    gf, gE, gW, ge = fx.pppm_compute_forces(at, eatom=True)
    tg = np.arange(n) if targets is None else np.asarray(targets)
    if len(probes):
        assert np.all(gf[probes] == 0.0) and np.all(ge[probes] == 0.0)
    assert np.abs(f).max() > 0 and scale > 0
    _compare(f"{tag} force", gf[tg], f, 1e-10 * np.abs(f).max())
    _compare(f"{tag} energy", gE, E, 1e-11 * scale)
    _compare(f"{tag} virial", gW, W, 1e-11 * scale)
    _compare(f"{tag} eatom", ge[tg], e, 1e-11 * scale)
    _compare(f"{tag} sum eatom = E", ge.sum(), gE, 1e-11 * scale)
    return (gf, gE, gW, ge), (f, E, W, e, scale, T)


@pytest.mark.parametrize("deck,mode,mesh,order", ref.ROWS)
def test_forces_energy_virial_match_the_mesh_reference_and_the_exact_sum(oracle, deck, mode, mesh, order):
    s, at, alist, blist, fx = _handle(deck, mode, mesh, order)
    assert bool(s.slabflag) == (mode == "slab")
    n = at.nlocal
    probes = _add_probes(s, at)
    tag = f"{deck}/{mode} {mesh} order {order}"
    (gf, gE, gW, ge), (f, E, W, e, scale, T) = check_against_reference(tag, oracle, s, at, fx, mesh, order, probes=probes)
    # the exact sum, within twice the error measured for the numpy mesh reference on this row (tests/test_pppm_force_math.py)
    x, q = np.ascontiguousarray(at.x[:n]), np.ascontiguousarray(at.q[:n])
    fe, Ee, We, ee, _ = ref.exact(s, x, q, T, np.arange(n))
    ferr, eerr = ref.rms(gf - fe) / ref.rms(fe), abs(gE - Ee) / scale
    mf, me = ref.MEASURED[(deck, mode, mesh, order)]
    print(f"{tag} vs exact: RMS force error {ferr:.3e} (reference {mf:.3e}), energy {eerr:.3e} (reference {me:.3e})")
    assert ferr <= 2 * mf and eerr <= 2 * me
    fx.close()


def test_forces_accumulate_and_null_outputs(oracle):
    s, at, alist, blist, fx = _handle("dilute", "ffield", (27, 24, 144), 5)
    scale = ref.reference(oracle, s, at, (27, 24, 144), 5, targets=np.arange(1))[4]
    n = at.nlocal
    f0, E0, W0, e0 = fx.pppm_compute_forces(at, eatom=True)
    assert np.abs(f0).max() > 0
    pre = np.random.default_rng(2).normal(size=(n, 3))
    f1 = fx.pppm_compute_forces(at, f=pre.copy())[0]
    _compare("pre-filled f", f1, pre + f0, 1e-10 * np.abs(f0).max())       # (the spread's atomic adds arrive in no fixed order)
    f2 = fx.pppm_compute_forces(at, f=f1.copy())[0]                         # calling twice adds twice
    _compare("twice", f2, pre + 2 * f0, 2e-10 * np.abs(f0).max())
    assert fx.pppm_compute_forces(at, energy=False, virial=False)[1:] == (None, None, None)
    fn, En, Wn, en = fx.pppm_compute_forces(at, forces=False, eatom=True)
    assert fn is None and abs(En - E0) <= 1e-11 * scale and np.abs(en - e0).max() <= 1e-11 * scale
    assert fx.pppm_compute_forces(at, forces=False, energy=False, virial=False) == (None, None, None, None)
    fx.close()


def test_contract_moved_atoms_kept_brick_cache_and_the_ewald_handle(oracle):
    deck, mode, mesh, order = "dilute", "ffield", (27, 24, 144), 5
    s, at, alist, blist, fx = _handle(deck, mode, mesh, order)
    n = at.nlocal
    f_plain = fx.pppm_compute_forces(at)[0]
    # keep_density on: an update leaves its electrolyte brick on the device; the forces are those of keep_density off
    fx.pppm_keep_density(True)
    fx.b_cal(at)
    f_keep = fx.pppm_compute_forces(at)[0]
    _compare("keep_density on / off", f_keep, f_plain, 1e-11 * np.abs(f_plain).max())
    # atoms moved WITHOUT an update (a pre_force that skips its update): the result is that of the atoms given, not of the kept brick
    ely = np.nonzero((at.echeck[:n] == 0) & (at.q[:n] != 0))[0]
    rng = np.random.default_rng(7)
    at.x[ely] += rng.uniform(2e-3, 5e-2, size=(len(ely), 3)) * rng.choice([-1.0, 1.0], size=(len(ely), 3))
    (gf, gE, gW, ge), _ = check_against_reference("moved atoms, no update", oracle, s, at, fx, mesh, order)
    assert np.abs(gf - f_keep).max() > 1e-6 * np.abs(f_keep).max()
    # the mesh-potential cache is conp_pppm_compute's: the per-atom entry gathers from it, no further spread or mesh solve
    n0 = fx.info().pppm_elyte_spreads
    sel = np.zeros(n, np.int32); sel[ely[:5]] = 1
    for i in ely[:5]:
        u = fx.pppm_particle_potential(at, int(i))
        # e_i = qs [q u_mesh / 2 - g q^2 / sqrt(pi) - ...], the entry returns -u_mesh + 2 g q / sqrt(pi)
        qi = at.q[i]
        Q = at.q[:n].sum()
        V = float(s.prd[0] * s.prd[1] * s.prd[2] * s.slab_volfactor)
        want = systems.QQRD2E * (-0.5 * qi * u - 0.5 * np.pi * qi * Q / (s.g_ewald ** 2 * V))
        assert ge[i] == pytest.approx(want, rel=1e-9, abs=1e-12)
    assert fx.info().pppm_elyte_spreads == n0
    fx.pppm_compute_forces(at)
    assert fx.info().pppm_elyte_spreads == n0 + 1
    fx.close()
    fe = FixConp(s)
    fe.init_lists(alist, blist)
    fe.setup_post_neighbor(at)
    with pytest.raises(ConpError) as e:
        fe.pppm_compute_forces(at)
    assert e.value.code == -2 and "conp_ewald_compute_forces" in str(e.value)          # CONP_ERR_STATE
    fe.close()


CHILD = r'''
import sys, numpy as np
sys.path.insert(0, {pkg!r}); sys.path.insert(0, {root!r})
from conp_amd import FixConp, neighbor, systems, capi
lib = capi.load_library()
lib.conp_debug_check_guards.restype = int
assert lib.conp_debug_check_guards() == 0, "guard zones are off"
s = systems.deck("il_onelayer", "slab")
at, alist, blist = neighbor.build_lists(s)
fx = FixConp(s, extra_args=["pppm"], pppm_mesh=(40, 45, 540), pppm_order=5)
fx.init_lists(alist, blist)
fx.setup_post_neighbor(at)
fx.setup_pre_force(at, 0, s.potdiff)
f, E, W, e = fx.pppm_compute_forces(at, eatom=True)
bad = lib.conp_debug_check_guards()
assert bad == 0, (bad, lib.conp_last_error().decode())
assert np.isfinite(f).all() and np.isfinite(e).all() and np.isfinite(W).all() and np.isfinite(E)
assert np.abs(f).max() > 0
fx.close()
print("GUARD_OK")
'''


def test_no_store_outside_the_buffers(tmp_path):
    script = tmp_path / "guard_child.py"
    script.write_text(CHILD.format(pkg=os.path.join(ROOT, "lammps-user-conp2_amd"), root=ROOT))
    env = dict(os.environ, CONP_GUARD="1")
    p = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "GUARD_OK" in p.stdout
