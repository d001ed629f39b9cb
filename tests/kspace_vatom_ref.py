"""numpy reference of the per-atom virial of both k-space force entries, straight from the definitions and
built on tests/ewald_force_ref.py and tests/pppm_force_ref.py.  tests/test_kspace_vatom_math.py guards these formulas (sum over the
atoms = the global virial, finite differences, mesh against exact sum) before the GPU tests use them to judge
conp_*_compute_forces_vatom[_device].

Component order everywhere: xx, yy, zz, xy, xz, yz.  Like PPPM::poisson_peratom the mesh reference does SIX separate backward
transforms and keeps their real parts; the library packs two fields into one complex transform after zeroing an off-diagonal
component's single-Nyquist planes (mesh_vatom_packed emulates that in numpy, so the rule itself is tested without a GPU)."""
import numpy as np

import pppm_force_ref as pref

PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def ewald_cweight(kv, ug, g):
    """w'_k = ug_k (1 / k^2 + 1 / (4 g^2)): the weights of Phi'"""
    k2 = (kv * kv).sum(axis=1)
    return ug * (1.0 / k2 + 0.25 / (g * g))


def ewald_phi_prime(S, r, kv, wp):
    """Phi'(r) = sum_k w'_k A(k; r) at fixed S, A = cos(k r) Re S_k + sin(k r) Im S_k; r: [m][3]"""
    ph = np.atleast_2d(r) @ kv.T
    return (wp * (np.cos(ph) * S.real + np.sin(ph) * S.imag)).sum(axis=1)


def ewald_vatom_parts(S, x, q, kv, ug, g, qs, targets, chunk=512):
    """(delta part [n], k_a k_b part [n][6]) of vatom_i,ab = qs q_i sum_k ug_k (delta_ab - 2 c_k k_a k_b) A_i(k) at `targets`:
    vatom = delta part on the diagonal + k_a k_b part"""
    targets = np.asarray(targets)
    wp = ewald_cweight(kv, ug, g)
    kk = np.stack([kv[:, a] * kv[:, b] for a, b in PAIRS], 1)
    d = np.zeros(len(targets))
    p = np.zeros((len(targets), 6))
    for a in range(0, len(targets), chunk):
        t = targets[a:a + chunk]
        ph = x[t] @ kv.T
        A = np.cos(ph) * S.real + np.sin(ph) * S.imag
        d[a:a + chunk] = A @ ug
        p[a:a + chunk] = -2.0 * ((A * wp) @ kk)
    qt = q[targets]
    return qs * qt * d, qs * qt[:, None] * p


def ewald_vatom(S, x, q, kv, ug, g, qs, targets):
    """vatom [len(targets)][6] of the exact Ewald sum (LAMMPS Ewald::compute); zero charges give exact zeros"""
    d, p = ewald_vatom_parts(S, x, q, kv, ug, g, qs, targets)
    v = p.copy()
    v[:, :3] += d[:, None]
    v[q[np.asarray(targets)] == 0] = 0.0
    return v


def _vg_phi(rho, T):
    """(phi = G rho^ (ifftn divides by N), the six vg_ab(k) arrays, Nyquist masks per axis)"""
    kx, ky, kz = pref.kvectors(T)
    KZ, KY, KX = np.meshgrid(kz, ky, kx, indexing="ij")
    K = (KX, KY, KZ)
    k2 = KX * KX + KY * KY + KZ * KZ
    with np.errstate(divide="ignore", invalid="ignore"):
        vt = np.where(k2 > 0, -2.0 * (1.0 / k2 + 0.25 / T["g"] ** 2), 0.0)
    phi = np.where(k2 > 0, T["greensfn"] * np.fft.fftn(rho), 0.0)
    vg = [(1.0 if a == b else 0.0) + vt * K[a] * K[b] for a, b in PAIRS]
    nx, ny, nz = T["mesh"]
    nyq = []
    for ax, n in ((2, nx), (1, ny), (0, nz)):        # array axes are (z, y, x)
        m = np.zeros((nz, ny, nx), bool)
        if n % 2 == 0:
            sl = [slice(None)] * 3
            sl[ax] = n // 2
            m[tuple(sl)] = True
        nyq.append(m)
    return phi, vg, nyq


def mesh_bricks(rho, T):
    """the six real bricks v_ab = Re IFFT[vg_ab phi]: six separate transforms, real parts (poisson_peratom)"""
    phi, vg, _ = _vg_phi(rho, T)
    return [np.fft.ifftn(v * phi).real for v in vg]


def mesh_bricks_packed(rho, T, zero_nyquist=True):
    """the library's scheme in numpy: (xx + i yy), (zz + i xy), (xz + i yz) through three complex transforms; an off-diagonal
    component is zeroed where exactly one of its two axes sits at its Nyquist index (zero_nyquist=False: what happens without)"""
    phi, vg, nyq = _vg_phi(rho, T)
    if zero_nyquist:
        for c, (a, b) in enumerate(PAIRS):
            if a != b:
                vg[c] = np.where(nyq[a] != nyq[b], 0.0, vg[c])
    out = [None] * 6
    for c0, c1 in ((0, 1), (2, 3), (4, 5)):
        z = np.fft.ifftn((vg[c0] + 1j * vg[c1]) * phi)
        out[c0], out[c1] = z.real, z.imag
    return out


def mesh_vatom(bricks, x, q, T, targets):
    """vatom_i,ab = qs q_i / 2 sum_stencil w v_ab (fieldforce_peratom; no slab term) at `targets`: [n][6]"""
    targets = np.asarray(targets)
    v = pref.gather(bricks, x[targets], T).T * (0.5 * T["qs"] * q[targets])[:, None]
    v[q[targets] == 0] = 0.0
    return v


def exact_vatom(s, x, q, T, targets):
    """vatom of the exact Ewald sum over the host k tables of `s` (pppm_force_ref.exact's k list)"""
    import ewald_force_ref as eref
    from conp_amd import capi
    kt = capi.host_ktables(s)
    kv = np.stack([kt["kxvecs"], kt["kyvecs"], kt["kzvecs"]], 1) * (2 * np.pi / T["prd"])
    S = eref.structure_factor(x, q, kv)
    return ewald_vatom(S, x, q, kv, np.asarray(kt["ug"]), T["g"], T["qs"], targets)


def reference(lib, s, at, mesh, order):
    """(vatom [nlocal][6], W [6], scale, T, x, q) of the mesh reference for the owned atoms of `at`"""
    import oracle_py
    pp = oracle_py.Pppm(lib, s, mesh, order, fast=True)
    T = pref.tables(lib, pp, s, mesh, order)
    pp.close()
    n = at.nlocal
    x, q = np.ascontiguousarray(at.x[:n]), np.ascontiguousarray(at.q[:n])
    rho = pref.spread(x, q, T)
    sol = pref.solve(rho, T)
    v = mesh_vatom(mesh_bricks(rho, T), x, q, T, np.arange(n))
    return v, T["qs"] * sol["wsum"], T["qs"] * sol["esum"], T, x, q


def rms_all(a):
    a = np.asarray(a, float)
    return float(np.sqrt((a * a).mean()))


# Measured on the CPU by tests/test_kspace_vatom_math.py with the electrode charges the oracle's pre_force leaves, per row of
# pppm_force_ref.ROWS: RMS over atoms and components of (mesh vatom - exact vatom) relative to the RMS of the exact vatom.  The GPU
# tests allow the library twice these against the exact sum (section 13's rule for the forces).
VATOM_MEASURED = {
    ("dilute", "ffield", (27, 24, 144), 5): 4.258e-4,
    ("il_onelayer", "ffield", (36, 40, 150), 4): 1.495e-4,
    ("dilute", "ffield", (32, 25, 160), 7): 1.287e-4,
    ("dilute", "slab", (27, 24, 432), 5): 6.985e-4,
}
# The largest |sum_i vatom_i,ab - W_ab| / (qs (V / 2) sum G |rho^|^2 / N^2) of the mesh reference over the four rows (rounding: the
# single-Nyquist planes cancel in W pair by pair and the real part drops them from v_ab); asserted with a 10x margin.
VATOM_SUM_RESIDUE = 3.7e-16
