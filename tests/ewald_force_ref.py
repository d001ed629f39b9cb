"""numpy reference of the exact Ewald reciprocal-space forces, energy, virial and per-atom energies, straight
from the definitions.  tests/test_ewald_force_math.py guards these formulas (finite differences) before the GPU tests use them to
judge conp_ewald_compute_forces."""
import numpy as np


def structure_factor(x, q, kv, chunk=512):
    """S_k = sum_j q_j e^{i k r_j} over the charged atoms"""
    src = np.nonzero(q != 0)[0]
    S = np.zeros(len(kv), complex)
    for a in range(0, len(src), chunk):
        j = src[a:a + chunk]
        S += q[j] @ np.exp(1j * (x[j] @ kv.T))
    return S


def ksum(S, ug):
    """sum_k ug_k |S_k|^2: the unsubtracted scale of the energy and the virial (without qqrd2e)"""
    return float((ug * (S.real ** 2 + S.imag ** 2)).sum())


def energy_virial(S, x, q, kv, ug, g, V, qs, slab=False, L=0.0):
    e_k = ug * (S.real ** 2 + S.imag ** 2)
    Q, Q2 = q.sum(), (q * q).sum()
    E = e_k.sum() - g * Q2 / np.sqrt(np.pi) - 0.5 * np.pi * Q * Q / (g * g * V)
    if slab:
        M, M2 = (q * x[:, 2]).sum(), (q * x[:, 2] ** 2).sum()
        E += 2 * np.pi * (M * M - Q * M2 - Q * Q * L * L / 12.0) / V
    k2 = (kv * kv).sum(axis=1)
    vt = -2.0 * (1.0 / k2 + 0.25 / (g * g)) * e_k
    W = np.array([(e_k + vt * kv[:, a] * kv[:, b]).sum() if a == b else (vt * kv[:, a] * kv[:, b]).sum()
                  for a, b in ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))])
    return qs * E, qs * W


def forces_eatom(S, x, q, kv, ug, g, V, qs, targets, slab=False, L=0.0, chunk=512):
    """f_i and e_i of the atoms `targets`; x, q: every owned atom (the slab sums run over all of them)"""
    targets = np.asarray(targets)
    f = np.zeros((len(targets), 3))
    u = np.zeros(len(targets))
    for a in range(0, len(targets), chunk):
        t = targets[a:a + chunk]
        ph = x[t] @ kv.T
        c, s = np.cos(ph), np.sin(ph)
        f[a:a + chunk] = ((2 * ug) * (s * S.real - c * S.imag)) @ kv
        u[a:a + chunk] = -((2 * ug) * (c * S.real + s * S.imag)).sum(axis=1)
    qt, zt = q[targets], x[targets, 2]
    Q = q.sum()
    f *= qt[:, None]
    u += 2 * g * qt / np.sqrt(np.pi)
    e = -0.5 * qt * u - 0.5 * np.pi * qt * Q / (g * g * V)
    if slab:
        M, M2 = (q * x[:, 2]).sum(), (q * x[:, 2] ** 2).sum()
        f[:, 2] += (-4 * np.pi / V) * qt * (M - Q * zt)
        e += (2 * np.pi / V) * qt * (zt * M - 0.5 * (M2 + Q * zt * zt) - Q * L * L / 12.0)
    return qs * f, qs * e


def handle_tables(fx, s):
    """(kv, ug, g, V, qs, slab, L) of a FixConp handle: the library's own k list and ug"""
    kt = fx.ktables()
    uk = np.array(fx.info().unitk)
    kv = np.stack([kt["kxvecs"], kt["kyvecs"], kt["kzvecs"]], 1) * uk
    from conp_amd import systems
    V = float(s.prd[0] * s.prd[1] * s.prd[2] * s.slab_volfactor)
    return dict(kv=kv, ug=np.asarray(kt["ug"]), g=float(s.g_ewald), V=V, qs=systems.QQRD2E, slab=bool(s.slabflag),
                L=float(s.prd[2] * s.slab_volfactor))
