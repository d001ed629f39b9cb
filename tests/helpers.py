"""shared drivers for the parity tests: the same System goes through the CPU oracle and through the HIP library"""
import numpy as np

from conp_amd import neighbor, systems
import oracle_py


def has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


class OracleRun:
    def __init__(self, lib, s, at, alist, blist, **kw):
        self.at = at
        self.q = at.q.copy()
        # the oracle writes charges into its own copy of q
        self.at_o = neighbor.Atoms(nlocal=at.nlocal, nghost=at.nghost, x=at.x, q=self.q, type=at.type, tag=at.tag,
                                   echeck=at.echeck, owner=at.owner)
        self.fx = oracle_py.Fix(lib, s, **kw)
        self.fx.set_atoms(self.at_o)
        self.fx.set_lists(alist, blist)
        self.fx.post_neighbor()

    def setup(self):
        assert self.fx.linalg_setup() == 0

    def pre_force(self, potdiff):
        self.fx.pre_force(potdiff)


def oracle_sk_and_b(s, at, alist, blist, rows=None):
    """the oracle's structure factors and b vector for the atoms as they are now: S(k) from KSpace.sincos_b over the charged
    electrolyte; b in eleall order, the k-space part from ele_trig + bbb (+ the slab term in slab geometry), the real-space part
    from blist_only().  `rows` (eleall
    indices) restricts the k-space part to those electrode atoms (the largest boxes); then b has len(rows) entries.
    Returns (sr, si, b, kspace) with the KSpace handle open (the caller closes it)."""
    lib = oracle_py.load(fast=True)
    lib.orc_set_threads(16)                                  # same arithmetic, OpenMP over k rows
    o = OracleRun(lib, s, at, alist, blist)                  # post_neighbor only: no A matrix needed for b
    m = o.fx.maps()
    loc = {int(t): i for i, t in enumerate(at.tag[:at.nlocal])}
    sel = np.arange(len(m["eleall2tag"])) if rows is None else np.asarray(rows)
    xele = np.array([at.x[loc[int(t)]] for t in m["eleall2tag"][sel]])
    ks = oracle_py.KSpace.from_system(lib, s)
    sr, si = ks.sincos_b(at.x, at.q, at.echeck, at.nlocal)
    csk, snk = ks.ele_trig(xele)
    b = ks.bbb(csk, snk, sr, si)
    if s.slabflag:                                           # the slab term of b_cal (orc_fix_b_cal)
        lib.orc_slabcorr(ks.h, at.nlocal, np.ascontiguousarray(at.x), np.ascontiguousarray(at.q),
                         np.ascontiguousarray(at.echeck, np.int32), len(xele), np.ascontiguousarray(xele), b)
    breal = np.zeros(len(m["eleall2tag"])); breal[m["ele2eleall"]] = o.fx.blist_only()
    b += breal[sel]
    o.fx.close()
    return sr, si, b, ks


def sk_err(sr_g, si_g, sr, si):
    """largest deviation of the GPU's structure factors from the reference's, relative to the reference's largest entry"""
    scale = max(np.abs(sr).max(), np.abs(si).max())
    return float(max(np.abs(sr_g - sr).max(), np.abs(si_g - si).max()) / scale)


def rel_err(a, b):
    a, b = np.asarray(a), np.asarray(b)
    den = max(np.max(np.abs(b)), 1e-300)
    return float(np.max(np.abs(a - b)) / den)


# erfc as the reference evaluates it (fix_conp.cpp:1446-1454 erfcr_sqrt; the coefficients are LAMMPS' pair-style constants, Abramowitz &
# Stegun 7.1.26): the polynomial is good to 1.5e-7 only, so it is part of the DEFINITION of A -- an exact erfc differs from the
# reference in the seventh digit of every near pair -- and so is its switch-off at an argument of 5.8
_AS_P, _AS_A = 0.3275911, (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
_ERFC_MAX = 5.8


def _erfc_over_r(a, rsq):
    """erfc(a r) / r in the reference's polynomial form, np.longdouble; 0 from a r = 5.8 on"""
    ar = a * np.sqrt(rsq)
    t = 1 / (1 + _AS_P * ar)
    poly = t * (_AS_A[0] + t * (_AS_A[1] + t * (_AS_A[2] + t * (_AS_A[3] + t * _AS_A[4]))))
    return np.where(ar < _ERFC_MAX, poly * np.exp(-ar * ar) / np.sqrt(rsq), 0)


def a_entries_from_definitions(s, at, ktables, info, pairs, *, eleall2tag, threads=16, kspace_only=False):
    """Entries A[i][j] of the electrode matrix for (i, j) in the permanent electrode numbering (`eleall2tag` gives the atoms),
    written from the definitions -- no neighbour list, no electrode tables, no recurrences, none of the library's or the
    oracle's loops:

        i != j:  sum_k 2 ug_k cos(k.(r_i - r_j))  +  [slab] 4 pi z_i z_j / V  +  sum_images [erfc(g r) - erfc(eta r / sqrt 2)] / r
        i == j:  sum_k 2 ug_k  -  2 g / sqrt(pi)  +  sqrt(2) eta / sqrt(pi)  +  [slab] 4 pi z_i^2 / V   (+ the atom's own images)

    k = (kx, ky, kz) * unitk and ug come from `ktables` (the half list), unitk and V (which includes slab_volfactor) from
    `info`; the images are all periodic copies (the periodic directions of `s`) with r^2 < cutsq[type_i][type_j] and
    r^2 < min(cut_coul, 5.8 / g)^2, as fix_conp.cpp:1242-1276 cuts them.  No qqrd2e anywhere.
    Everything is evaluated and summed in np.longdouble (64-bit mantissa); the diagonal's sum_k with math.fsum.  The k sum is
    `kspace_only`: what the k-space provider alone contributes (km_ewald.cpp:584-666) -- no images and no eta term.  The k sum is
    the direct one, term by term: cos(k.d) is taken as Re[e^{i kx tx} e^{i ky ty} e^{i kz tz}] with every factor a direct
    cos / sin of n * t (t = unitk * d), and the terms are added up as a contraction of the dense array 2 ug[kx][ky][kz]
    (zero where the half list has no vector) with those factors.  `threads` only spreads batches of pairs."""
    import math
    from concurrent.futures import ThreadPoolExecutor
    LD = np.longdouble
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    unitk = np.array([info.unitk[0], info.unitk[1], info.unitk[2]], dtype=np.float64)
    volume = float(info.volume)
    prd = np.asarray(s.prd, dtype=np.float64)
    assert np.allclose(unitk, 2 * np.pi / (prd * np.array([1.0, 1.0, s.slab_volfactor])), rtol=1e-14)
    assert math.isclose(volume, prd[0] * prd[1] * prd[2] * s.slab_volfactor, rel_tol=1e-14)
    loc = {int(t): i for i, t in enumerate(at.tag[:at.nlocal])}
    rows = np.array([loc[int(t)] for t in eleall2tag])
    xe, te = at.x[rows].astype(LD), at.type[rows]
    kx, ky, kz = (np.asarray(ktables[n], dtype=np.int64) for n in ("kxvecs", "kyvecs", "kzvecs"))
    ug = np.asarray(ktables["ug"], dtype=np.float64)
    out = np.zeros(len(pairs), dtype=LD)
    diag = pairs[:, 0] == pairs[:, 1]
    off = np.nonzero(~diag)[0]
    # ---- k space, off the diagonal
    lo = np.array([kx.min(), ky.min(), kz.min()]); dim = np.array([kx.max(), ky.max(), kz.max()]) - lo + 1
    W = np.zeros(dim, dtype=LD)
    np.add.at(W, (kx - lo[0], ky - lo[1], kz - lo[2]), 2 * ug.astype(LD))
    W2 = W.reshape(dim[0] * dim[1], dim[2])
    nvec = [np.arange(lo[c], lo[c] + dim[c]).astype(LD) for c in range(3)]
    d_off = xe[pairs[off, 0]] - xe[pairs[off, 1]]                       # exact: differences of float64 in extended precision

    def ksum(sl):
        th = d_off[sl] * unitk.astype(LD)                               # [P][3]
        ph = [th[:, c, None] * nvec[c][None, :] for c in range(3)]     # n * t, then cos / sin of it: no recurrence
        cz, sz = np.cos(ph[2]), np.sin(ph[2])
        c1, s1 = W2 @ cz.T, W2 @ sz.T                                   # sum over kz: [nx ny][P]
        cxy = (np.cos(ph[0])[:, :, None] * np.cos(ph[1])[:, None, :] - np.sin(ph[0])[:, :, None] * np.sin(ph[1])[:, None, :])
        sxy = (np.sin(ph[0])[:, :, None] * np.cos(ph[1])[:, None, :] + np.cos(ph[0])[:, :, None] * np.sin(ph[1])[:, None, :])
        P = len(th)
        return (cxy.reshape(P, -1) * c1.T - sxy.reshape(P, -1) * s1.T).sum(axis=1)

    batch = 64
    slices = [slice(b, min(b + batch, len(off))) for b in range(0, len(off), batch)]
    with ThreadPoolExecutor(max(1, threads)) as pool:
        for sl, v in zip(slices, pool.map(ksum, slices)):
            out[off[sl]] = v
    # ---- the diagonal's k sum and self terms
    pi = 4 * np.arctan(LD(1))
    sqrt_pi = np.sqrt(pi)
    g, eta = LD(s.g_ewald), LD(s.eta)
    out[diag] = LD(math.fsum(2.0 * ug)) - 2 * g / sqrt_pi + (0 if kspace_only else np.sqrt(LD(2)) * eta / sqrt_pi)
    # ---- slab term
    if s.slabflag == 1:
        out += 4 * pi * xe[pairs[:, 0], 2] * xe[pairs[:, 1], 2] / LD(volume)
    if kspace_only:
        return out.astype(np.float64)
    # ---- real space: every periodic image inside the cutoffs (the atom's own images on the diagonal, never r = 0)
    cutsq = s.cutsq_table()[te[pairs[:, 0]], te[pairs[:, 1]]]
    cut_coulsq = min(s.cutoff ** 2, _ERFC_MAX ** 2 / s.g_ewald ** 2)
    nmax = [int(np.ceil(s.cutoff / prd[c])) + 1 if s.periodic[c] else 0 for c in range(3)]
    d = xe[pairs[:, 0]] - xe[pairs[:, 1]]
    for n0 in range(-nmax[0], nmax[0] + 1):
        for n1 in range(-nmax[1], nmax[1] + 1):
            for n2 in range(-nmax[2], nmax[2] + 1):
                dd = d + np.array([n0, n1, n2]).astype(LD) * prd.astype(LD)
                rsq = (dd * dd).sum(axis=1)
                inside = (rsq > 0) & (rsq < cutsq) & (rsq < cut_coulsq)
                r2 = np.where(inside, rsq, LD(1))
                out += np.where(inside, _erfc_over_r(g, r2) - _erfc_over_r(eta / np.sqrt(LD(2)), r2), 0)
    return out.astype(np.float64)


def push_outside(s, at, seed=3):
    """positions as LAMMPS leaves them between re-neighbourings: twelve charged electrolyte atoms put up to 1 A outside the box (two
    per face), unwrapped, and three more exactly on boxhi, one per direction; the ghosts move with their owners.  Returns the indices
    of the moved atoms (the three on boxhi last)."""
    rng = np.random.default_rng(seed)
    n = at.nlocal
    cand = np.nonzero((at.echeck[:n] == 0) & (at.q[:n] != 0))[0]
    moved = rng.choice(cand, 15, replace=False)
    d = np.zeros((n, 3))
    for k, i in enumerate(moved):
        c = k % 3
        if k >= 12:
            target = s.boxhi[c]
        elif (k // 3) % 2:
            target = s.boxhi[c] + rng.uniform(0.05, 1.0)
        else:
            target = s.boxlo[c] - rng.uniform(0.05, 1.0)
        d[i, c] = target - at.x[i, c]
        at.x[i, c] = target
    at.x[n:] += d[at.owner[n:]]
    return [int(i) for i in moved]
