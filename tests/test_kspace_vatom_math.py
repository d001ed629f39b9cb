"""No GPU: the numpy reference of tests/kspace_vatom_ref.py before it judges the per-atom virial of the library
(tests/test_gpu_kspace_vatom*.py).

(1) Ewald: sum_i vatom_i = W of ewald_force_ref.energy_virial (1e-12 of qs sum ug |S|^2), on seeded charges in a random box and on
    the dilute deck with the oracle's electrode charges;  (2) Ewald: the k_a k_b part, -2 qs q_i sum_k w'_k k_a k_b A_i(k), equals
    2 qs q_i Hess_ab Phi'_i (d2 A = -k_a k_b A), by central second differences;
    (3) mesh: sum_i vatom_i against W of pppm_force_ref.energy_virial on the four ROWS meshes (even and odd lengths on every axis);
    (4) mesh: the packed scheme of the library (three complex transforms, single-Nyquist planes of the off-diagonal components
    zeroed) equals the six separate transforms to rounding, and does NOT without the zeroing;  (5) mesh against the exact sum, the
    table VATOM_MEASURED.

Measured here (CPU), mesh against exact sum = RMS over atoms and components of the difference / RMS of the exact vatom; residue =
max_ab |sum_i vatom_i,ab - W_ab| / scale:
    deck         mode    mesh            order   mesh vs exact   residue     packed vs separate   packed, no zeroing
    dilute       ffield  27 x 24 x 144   5       4.258e-4        1.506e-16   1.412e-17            4.004e-9
    il_onelayer  ffield  36 x 40 x 150   4       1.495e-4        3.652e-16   9.129e-17            9.129e-17
    dilute       ffield  32 x 25 x 160   7       1.287e-4        7.528e-17   9.410e-18            2.832e-10
    dilute       slab    27 x 24 x 432   5       6.985e-4        7.528e-17   1.176e-17            1.335e-9
The residue is rounding: no Nyquist term survives in either side (in W the single-Nyquist planes cancel pair by pair).  On
il_onelayer's mesh the spectrum on those planes is itself at rounding level, so only the three dilute rows can tell a build without
the zeroing from one with it; they do so by 30x to 400x the GPU tests' bound of 1e-11.  Ewald finite differences: 1.8e-7 / 1.2e-7.
"""
import numpy as np
import pytest

import ewald_force_ref as eref
import kspace_vatom_ref as vref
import pppm_force_ref as pref
from test_ewald_force_math import QS, _box, _klist
from test_pppm_force_math import _row


@pytest.mark.parametrize("slab", [False, True])
def test_ewald_vatom_sums_to_the_global_virial(slab):
    x, q, prd, volfac = _box(slab)
    g = 0.35
    kv, ug, V = _klist(prd, volfac, g)
    S = eref.structure_factor(x, q, kv)
    W = eref.energy_virial(S, x, q, kv, ug, g, V, QS)[1]
    v = vref.ewald_vatom(S, x, q, kv, ug, g, QS, np.arange(40))
    scale = QS * eref.ksum(S, ug)
    res = np.abs(v.sum(axis=0) - W).max() / scale
    print(f"slab {slab}: max |sum_i vatom_i - W| / scale = {res:.3e}")
    assert res <= 1e-12
    assert np.all(v[:4] == 0.0)                                # probes
    # without the delta_ab term the diagonal misses the whole k sum
    d, p = vref.ewald_vatom_parts(S, x, q, kv, ug, g, QS, np.arange(40))
    assert np.abs(p.sum(axis=0) - W)[:3].min() > 0.1 * scale
    assert abs(d.sum() - scale) <= 1e-12 * scale


def test_ewald_vatom_sums_to_the_global_virial_on_the_dilute_deck(oracle):
    s, at, x, q, pp, T, rho, sol = _row(oracle, *pref.ROWS[0])
    from conp_amd import capi
    kt = capi.host_ktables(s)
    kv = np.stack([kt["kxvecs"], kt["kyvecs"], kt["kzvecs"]], 1) * (2 * np.pi / T["prd"])
    ug = np.asarray(kt["ug"])
    S = eref.structure_factor(x, q, kv)
    W = eref.energy_virial(S, x, q, kv, ug, T["g"], T["V"], T["qs"])[1]
    v = vref.ewald_vatom(S, x, q, kv, ug, T["g"], T["qs"], np.arange(at.nlocal))
    assert np.abs(v.sum(axis=0) - W).max() <= 1e-12 * T["qs"] * eref.ksum(S, ug)


@pytest.mark.parametrize("slab", [False, True])
def test_ewald_kk_part_is_the_hessian_of_phi_prime(slab):
    """vatom_kk,ab = -2 qs q_i sum_k w'_k k_a k_b A_i(k) = 2 qs q_i d2 Phi'_i / dr_a dr_b at fixed S (d2 A = -k_a k_b A): minus the
    Hessian of -2 qs q_i Phi'_i.  Central second differences at h = 1e-3: truncation h^2 k^2 / 12 ~ 5e-7 relative with |k| <= 2.4,
    rounding eps / h^2 ~ 1e-10 of Phi' -- asserted at 5e-6 of the largest entry (measured: see the print)."""
    x, q, prd, volfac = _box(slab)
    g = 0.35
    kv, ug, V = _klist(prd, volfac, g)
    S = eref.structure_factor(x, q, kv)
    wp = vref.ewald_cweight(kv, ug, g)
    atoms = np.array([4, 9, 17, 25, 39])
    _, p = vref.ewald_vatom_parts(S, x, q, kv, ug, g, QS, atoms)
    h = 1e-3
    E = np.eye(3) * h
    fd = np.zeros_like(p)
    for n, i in enumerate(atoms):
        r = x[i]
        for c, (a, b) in enumerate(vref.PAIRS):
            pts = np.array([r + E[a] + E[b], r + E[a] - E[b], r - E[a] + E[b], r - E[a] - E[b]])
            f = vref.ewald_phi_prime(S, pts, kv, wp)
            fd[n, c] = 2.0 * QS * q[i] * (f[0] - f[1] - f[2] + f[3]) / (4 * h * h)
    err = np.abs(p - fd).max() / np.abs(fd).max()
    print(f"slab {slab}: k_a k_b part against the finite-difference Hessian: {err:.3e}")
    assert err <= 5e-6


@pytest.mark.parametrize("deck,mode,mesh,order", pref.ROWS)
def test_mesh_vatom_sums_to_the_global_virial_and_packing_needs_the_nyquist_rule(oracle, deck, mode, mesh, order):
    s, at, x, q, pp, T, rho, sol = _row(oracle, deck, mode, mesh, order)
    n = at.nlocal
    scale = T["qs"] * sol["esum"]
    W = pref.energy_virial(sol, x, q, T)[1]
    bricks = vref.mesh_bricks(rho, T)
    v = vref.mesh_vatom(bricks, x, q, T, np.arange(n))
    res = np.abs(v.sum(axis=0) - W).max() / scale
    packed = vref.mesh_vatom(vref.mesh_bricks_packed(rho, T), x, q, T, np.arange(n))
    leaky = vref.mesh_vatom(vref.mesh_bricks_packed(rho, T, zero_nyquist=False), x, q, T, np.arange(n))
    dp, dl = np.abs(packed - v).max() / scale, np.abs(leaky - v).max() / scale
    print(f"{deck} {mode} {mesh} order {order}: residue {res:.3e}, packed vs separate {dp:.3e}, without the zeroing {dl:.3e}")
    assert res <= 10 * vref.VATOM_SUM_RESIDUE
    assert np.all(v[q == 0] == 0.0)
    assert dp <= 1e-13                                         # the packed scheme IS the six real parts, to rounding
    if deck == "dilute":
        assert dl > 2e-10                                      # above the GPU tests' bound (1e-11): a build without the rule fails them
    # without the delta_ab term the diagonal misses the whole mesh sum
    assert np.abs((v.sum(axis=0) - W)[:3] - (-scale)).max() > 0.1 * scale


@pytest.mark.parametrize("deck,mode,mesh,order", pref.ROWS)
def test_mesh_vatom_against_the_exact_sum_is_the_recorded_one(oracle, deck, mode, mesh, order):
    """measures VATOM_MEASURED (the GPU tests' yardstick against the exact sum)"""
    s, at, x, q, pp, T, rho, sol = _row(oracle, deck, mode, mesh, order)
    n = at.nlocal
    v = vref.mesh_vatom(vref.mesh_bricks(rho, T), x, q, T, np.arange(n))
    ve = vref.exact_vatom(s, x, q, T, np.arange(n))
    err = vref.rms_all(v - ve) / vref.rms_all(ve)
    print(f"{deck} {mode} {mesh} order {order}: mesh vatom against the exact sum {err:.3e}")
    assert err == pytest.approx(vref.VATOM_MEASURED[(deck, mode, mesh, order)], rel=2e-3)
    assert 1e-6 < err < 1e-2
