"""No GPU: the numpy reference of tests/ewald_force_ref.py against finite differences of its own energy, before it judges the
library (tests/test_gpu_ewald_forces*.py).  A 40-atom random box, periodic and slab."""
import numpy as np
import pytest

import ewald_force_ref as ref

QS = 332.06371


def _box(slab):
    rng = np.random.default_rng(5)
    prd = np.array([11.0, 9.0, 14.0])
    volfac = 3.0 if slab else 1.0
    x = rng.random((40, 3)) * prd
    q = rng.normal(size=40)
    q[:4] = 0.0                                   # probes
    q[4:] -= q[4:].mean() - 0.01                  # a small net charge: the Q terms are exercised
    return x, q, prd, volfac


def _klist(prd, volfac, g, kcut=2.4):
    """a half list: one of every (k, -k) pair with |k| <= kcut"""
    uk = 2 * np.pi / (prd * np.array([1.0, 1.0, volfac]))
    nmax = np.ceil(kcut / uk).astype(int)
    out = []
    for a in range(0, nmax[0] + 1):
        for b in range(-nmax[1], nmax[1] + 1):
            for c in range(-nmax[2], nmax[2] + 1):
                if (a, b, c) == (0, 0, 0) or (a == 0 and (b < 0 or (b == 0 and c < 0))):
                    continue
                k = np.array([a, b, c]) * uk
                if k @ k <= kcut * kcut:
                    out.append(k)
    kv = np.array(out)
    V = prd.prod() * volfac
    k2 = (kv * kv).sum(axis=1)
    return kv, 4 * np.pi / V * np.exp(-k2 / (4 * g * g)) / k2, V


def _energy(x, q, kv, ug, g, V, slab, L):
    S = ref.structure_factor(x, q, kv)
    return ref.energy_virial(S, x, q, kv, ug, g, V, QS, slab, L)[0]


@pytest.mark.parametrize("slab", [False, True])
def test_reference_forces_are_the_gradient_of_the_reference_energy(slab):
    x, q, prd, volfac = _box(slab)
    g = 0.35
    kv, ug, V = _klist(prd, volfac, g)
    L = prd[2] * volfac
    S = ref.structure_factor(x, q, kv)
    E, W = ref.energy_virial(S, x, q, kv, ug, g, V, QS, slab, L)
    allat = np.arange(40)
    f, e = ref.forces_eatom(S, x, q, kv, ug, g, V, QS, allat, slab, L)
    # f = -dE/dr by central differences (h^2 f''' / 6 ~ 1e-8 relative at h = 1e-4 with |k| <= 2.4; rounding E eps / h ~ 1e-9)
    h = 1e-4
    fd = np.zeros_like(f)
    for i in range(40):
        for c in range(3):
            xp, xm = x.copy(), x.copy()
            xp[i, c] += h; xm[i, c] -= h
            fd[i, c] = -(_energy(xp, q, kv, ug, g, V, slab, L) - _energy(xm, q, kv, ug, g, V, slab, L)) / (2 * h)
    assert np.abs(f - fd).max() <= 1e-6 * np.abs(fd).max()
    assert np.all(f[:4] == 0.0)                                # probes
    assert abs(e.sum() - E) <= 1e-12 * QS * ref.ksum(S, ug)
    if not slab:
        assert np.abs(f.sum(axis=0)).max() <= 1e-12 * np.abs(f).sum()


@pytest.mark.parametrize("slab", [False, True])
def test_reference_virial_trace_is_the_volume_derivative_of_the_k_sum(slab):
    """A uniform scaling r -> s r, k -> k / s, V -> s^3 V leaves every S_k as it is.  With g FIXED the k sum E_k = qs sum ug |S|^2
    changes through ug alone, and -3 V dE_k/dV = -s dE_k/ds = qs sum ug |S|^2 (1 - k^2 / (2 g^2)) = W_xx + W_yy + W_zz: the virial
    formula is that of the k sum at fixed g (the self term does not depend on V; were g scaled with 1 / s, E_k would be
    homogeneous of degree -1 and the derivative would be E_k itself, which is not what the formula states)."""
    x, q, prd, volfac = _box(slab)
    g = 0.35
    kv, ug, V = _klist(prd, volfac, g)
    S = ref.structure_factor(x, q, kv)
    W = ref.energy_virial(S, x, q, kv, ug, g, V, QS)[1]

    def ek(s):
        k2 = (kv * kv).sum(axis=1) / (s * s)
        return QS * ref.ksum(S, 4 * np.pi / (V * s ** 3) * np.exp(-k2 / (4 * g * g)) / k2)
    h = 1e-5
    fd = -(ek(1 + h) - ek(1 - h)) / (2 * h)
    assert abs(W[:3].sum() - fd) <= 1e-8 * ek(1.0)
