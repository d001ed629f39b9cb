"""-m gpu: conp_ewald_compute_forces -- the exact Ewald reciprocal-space forces, energy, virial and per-atom energies on the device
(DESIGN.md section 12): what a KSpace style's compute() does after the charge update.

(1) against the numpy reference of tests/ewald_force_ref.py (guarded by tests/test_ewald_force_math.py) summed over the library's own
    k list, on ALL owned atoms, zero-charge probes included;  (2) the headline box, S from the oracle's OpenMP sincos_b, forces on a
    sample;  (3) accumulation into f, the cache of S, the pppm handle refuses;  (4) guard zones.
Bounds: forces 1e-10 max|f| (the potential's 1e-11 of tests/test_gpu_ewald_potential.py times 10 for the k-weighted sum); energy,
virial and per-atom energies 1e-11 of qs sum ug |S|^2, the unsubtracted scale (the self term cancels most of E).
Ranks: tests/test_gpu_ewald_forces_ranks.py; the glue: tests/test_gpu_ewald_forces_glue.py."""
import os
import subprocess
import sys

import numpy as np
import pytest

import ewald_force_ref as ref
from conp_amd import ConpError, FixConp, neighbor, systems
from test_gpu_ewald_potential import _add_probes, _handle, _system

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _compare(tag, got, want, bound):
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    print(f"{tag}: max error {err:.3e}, bound {bound:.3e} ({err / bound:.3g} of it)")
    assert err <= bound, (tag, err, bound)


@pytest.mark.parametrize("name,mode", [("small", "slab"), ("small", "ffield"), ("dilute", "slab"), ("dilute", "ffield"),
                                       ("il_onelayer", "slab")])
def test_forces_energy_virial_match_the_definitions(name, mode):
    s = _system(name, mode)
    at, alist, blist, fx = _handle(s)
    n = at.nlocal
    probes = _add_probes(s, at)
    T = ref.handle_tables(fx, s)
    x, q = np.ascontiguousarray(at.x[:n]), np.ascontiguousarray(at.q[:n])
    S = ref.structure_factor(x, q, T["kv"])
    E, W = ref.energy_virial(S, x, q, T["kv"], T["ug"], T["g"], T["V"], T["qs"], T["slab"], T["L"])
    f, e = ref.forces_eatom(S, x, q, T["kv"], T["ug"], T["g"], T["V"], T["qs"], np.arange(n), T["slab"], T["L"])
    gf, gE, gW, ge = fx.ewald_forces(at, eatom=True)
    scale = T["qs"] * ref.ksum(S, T["ug"])
    assert np.all(gf[probes] == 0.0) and np.all(ge[probes] == 0.0)
    _compare(f"{name}/{mode} force", gf, f, 1e-10 * np.abs(f).max())
    _compare(f"{name}/{mode} energy", gE, E, 1e-11 * scale)
    _compare(f"{name}/{mode} virial", gW, W, 1e-11 * scale)
    _compare(f"{name}/{mode} eatom", ge, e, 1e-11 * scale)
    fx.close()


@pytest.mark.parametrize("name", ["headline", "headline_slab"])
def test_headline_box_matches_the_oracle_structure_factor(name):
    """synthetic_fast 4096 / 32768 after an update of the z-window form: S from the oracle's OpenMP sincos_b with an all-zero echeck
    (every atom charged), forces from the definitions on 256 electrode atoms, 256 electrolyte atoms and the probes; E and W from
    that S.  The library computes the forces of all 36 864 atoms in the call."""
    import oracle_py
    s = _system(name, "slab" if name == "headline_slab" else "ffield")
    at, alist, blist, fx = _handle(s)
    assert fx.info().zn_cols > 0
    n = at.nlocal
    probes = _add_probes(s, at)
    rng = np.random.default_rng(3)
    ele = np.nonzero(at.echeck[:n] != 0)[0]
    ely = np.nonzero((at.echeck[:n] == 0) & (at.q[:n] != 0))[0]
    tg = np.concatenate([rng.choice(ele, 256, replace=False), rng.choice(ely, 256, replace=False), probes])
    gf, gE, gW, ge = fx.ewald_forces(at, eatom=True)
    lib = oracle_py.load(fast=True)
    ks = oracle_py.KSpace.from_system(lib, s)
    x, q = np.ascontiguousarray(at.x[:n]), np.ascontiguousarray(at.q[:n])
    sr, si = ks.sincos_b(x, q, np.zeros(n, np.int32), n)
    S = np.asarray(sr) + 1j * np.asarray(si)
    T = ref.handle_tables(fx, s)
    E, W = ref.energy_virial(S, x, q, T["kv"], T["ug"], T["g"], T["V"], T["qs"], T["slab"], T["L"])
    f, e = ref.forces_eatom(S, x, q, T["kv"], T["ug"], T["g"], T["V"], T["qs"], tg, T["slab"], T["L"], chunk=64)
    scale = T["qs"] * ref.ksum(S, T["ug"])
    assert np.all(gf[probes] == 0.0)
    _compare(f"{name} force (sample)", gf[tg], f, 1e-10 * np.abs(f).max())
    _compare(f"{name} energy", gE, E, 1e-11 * scale)
    _compare(f"{name} virial", gW, W, 1e-11 * scale)
    _compare(f"{name} eatom (sample)", ge[tg], e, 1e-11 * scale)
    if not s.slabflag:
        _compare(f"{name} net force", np.abs(gf.sum(axis=0)).max(), 0.0, 1e-9 * np.abs(gf).sum())
    ks.close(); fx.close()


def test_forces_accumulate_and_the_structure_factor_is_cached():
    s = _system("dilute", "ffield")
    at, alist, blist, fx = _handle(s)
    n = at.nlocal
    f0, E0, W0, e0 = fx.ewald_forces(at, eatom=True)
    assert np.abs(f0).max() > 0
    # a pre-filled f is added to
    pre = np.random.default_rng(2).normal(size=(n, 3))
    f1 = fx.ewald_forces(at, f=pre.copy())[0]
    assert np.array_equal(f1, pre + f0)
    # after a collective entry the cache serves: bit-identical results
    fx.ewald_compute(at)
    f2, E2, W2, e2 = fx.ewald_forces(at, eatom=True)
    assert np.array_equal(f2, f0) and E2 == E0 and np.array_equal(W2, W0) and np.array_equal(e2, e0)
    # the contract of the C entry: the cached S is that of the x and q the collective entry saw, and only valid for those.  Two
    # charges changed WITHOUT an update: the call still contracts the cached S (of the old charges) -- with the new q_i as the
    # prefactors -- and not the S of the charges it is given.  (A KSpace style, whose atoms move between updates, therefore
    # refreshes S itself: tests/test_gpu_ewald_forces_glue.py.)
    T = ref.handle_tables(fx, s)
    x, q_old = np.ascontiguousarray(at.x[:n]), at.q[:n].copy()
    S_old = ref.structure_factor(x, q_old, T["kv"])
    q_keep = at.q.copy()
    ely = np.nonzero((at.echeck[:n] == 0) & (at.q[:n] != 0))[0]
    at.q[ely[0]] *= 1.5; at.q[ely[1]] -= 0.5 * q_keep[ely[0]]
    q_new = np.ascontiguousarray(at.q[:n])
    fc = fx.ewald_forces(at)[0]
    f_cached, _ = ref.forces_eatom(S_old, x, q_new, T["kv"], T["ug"], T["g"], T["V"], T["qs"], np.arange(n))
    f_fresh, _ = ref.forces_eatom(ref.structure_factor(x, q_new, T["kv"]), x, q_new, T["kv"], T["ug"], T["g"], T["V"], T["qs"], np.arange(n))
    assert np.abs(f_cached - f_fresh).max() > 1e-6 * np.abs(f_fresh).max()
    _compare("cached S force", fc, f_cached, 1e-10 * np.abs(f_cached).max())
    at.q[:] = q_keep
    # an update drops the cache: the next call forms S of the atoms it is given
    fx.b_cal(at)
    at.q[ely[0]] *= 1.5; at.q[ely[1]] -= 0.5 * q_keep[ely[0]]
    f3, E3 = fx.ewald_forces(at)[:2]
    x, q = np.ascontiguousarray(at.x[:n]), np.ascontiguousarray(at.q[:n])
    S = ref.structure_factor(x, q, T["kv"])
    f, _ = ref.forces_eatom(S, x, q, T["kv"], T["ug"], T["g"], T["V"], T["qs"], np.arange(n))
    assert np.abs(f3 - f0).max() > 1e-6 * np.abs(f0).max()
    _compare("re-formed S force", f3, f, 1e-10 * np.abs(f).max())
    # outputs that were not asked for
    assert fx.ewald_forces(at, energy=False, virial=False)[1:] == (None, None, None)
    fx.close()
    fp = FixConp(s, extra_args=["pppm"], pppm_mesh=(27, 24, 144), pppm_order=5)
    fp.init_lists(alist, blist)
    fp.setup_post_neighbor(at)
    with pytest.raises(ConpError) as e:
        fp.ewald_forces(at)
    assert "conp_pppm_compute" in str(e.value)
    fp.close()


CHILD = r'''
import sys, numpy as np
sys.path.insert(0, {pkg!r}); sys.path.insert(0, {root!r})
from conp_amd import FixConp, neighbor, systems, capi
lib = capi.load_library()
lib.conp_debug_check_guards.restype = int
assert lib.conp_debug_check_guards() == 0, "guard zones are off"
s = systems.deck("il_onelayer", "slab")
at, alist, blist = neighbor.build_lists(s)
fx = FixConp(s)
fx.init_lists(alist, blist)
fx.setup_post_neighbor(at)
fx.setup_pre_force(at, 0, s.potdiff)
f, E, W, e = fx.ewald_forces(at, eatom=True)
bad = lib.conp_debug_check_guards()
assert bad == 0, (bad, lib.conp_last_error().decode())
assert np.isfinite(f).all() and np.isfinite(e).all() and np.isfinite(W).all() and np.isfinite(E)
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
