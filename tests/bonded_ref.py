"""numpy reference (np.longdouble) of harmonic bonds and angles, straight from the definition in include/conp_hip.h
(conp_bonded_compute; LAMMPS bond_harmonic.cpp, angle_harmonic.cpp, Bond::ev_tally, Angle::ev_tally @ 27May2021).

Two things are part of the definition, because dr = r - r0 and acos amplify their rounding without bound: the closest image is
float64 as written, and r, r1, r2 and c are the float64 values formed as written.  Everything downstream is longdouble.

reference(...) returns the results (f, eng, W, eatom, vatom) and the cancellation-free magnitudes the bounds of the GPU tests are
stated against -- every term replaced by its absolute value and every difference by the sum of its operands' magnitudes
(dr -> r + |r0|, dtheta -> acos(c) + |theta0|): A[nall][3], E_abs[2], W_abs[6], eatom_abs[nall], vatom_abs[nall][6].
restate64(...) is the same arithmetic in float64 in the kernels' order; the builders below make the inputs of the GPU tests."""
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
TOL = 1e-12
# launch shapes of conp_bonded.hip, restated (tests/test_bonded_ref_math.py compares them with csrc/conp_kernels.h)
BLOCK = 256       # threads of a workgroup: one term each (term kernel), one atom each (gather kernel)
FINISH = 256      # threads of the finishing workgroup: from BLOCK * FINISH terms on a thread adds a second row
TERM_W = 13
THIRD = 1.0 / 3.0

# bond_coeff K r0 (three types) and angle_coeff K theta0 (two types, degrees in the deck, radians at the ABI)
PARAMS = SimpleNamespace(bond_k=np.array([450.0, 320.0, 553.0]), bond_r0=np.array([1.0, 1.1, 1.25]),
                         angle_k=np.array([55.0, 75.0]), angle_theta0=np.deg2rad(np.array([104.52, 112.0])))


def closest_image(xa, xb, prd):
    """x_b seen from x_a, float64 as written -> (x_b', s); the product first, then the sum, also for s = 0"""
    xa, xb, prd = np.asarray(xa, np.float64), np.asarray(xb, np.float64), np.asarray(prd, np.float64)
    d = xa - xb
    h = prd / 2
    s = np.where(d > h, 1.0, np.where(d < -h, -1.0, 0.0)) * (prd > 0)
    shift = s * prd
    return np.where(prd > 0, xb + shift, xb), s.astype(np.int64)


def _lists(bonds, angles):
    b = np.asarray(bonds if bonds is not None else np.zeros((0, 3)), dtype=np.int64).reshape(-1, 3)
    a = np.asarray(angles if angles is not None else np.zeros((0, 4)), dtype=np.int64).reshape(-1, 4)
    return b, a


def _six(u, v):
    """(ux vx, uy vy, uz vz, ux vy, ux vz, uy vz)"""
    return np.stack([u[:, 0] * v[:, 0], u[:, 1] * v[:, 1], u[:, 2] * v[:, 2], u[:, 0] * v[:, 1], u[:, 0] * v[:, 2], u[:, 1] * v[:, 2]], 1)


def _geometry(x, bonds, angles, prd):
    """the float64 part of the definition: images, r of a bond, r1, r2 and c of an angle"""
    x = np.asarray(x, dtype=np.float64)
    g = SimpleNamespace()
    x1, (x2, g.sb) = x[bonds[:, 0]], closest_image(x[bonds[:, 0]], x[bonds[:, 1]], prd)
    d = x1 - x2
    g.bx1, g.bx2 = x1, x2
    g.r = np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])
    xc = x[angles[:, 1]]
    (xa, g.s1), (xb, g.s3) = closest_image(xc, x[angles[:, 0]], prd), closest_image(xc, x[angles[:, 2]], prd)
    d1, d2 = xa - xc, xb - xc
    g.ac, g.a1, g.a3 = xc, xa, xb
    g.r1 = np.sqrt(d1[:, 0] * d1[:, 0] + d1[:, 1] * d1[:, 1] + d1[:, 2] * d1[:, 2])
    g.r2 = np.sqrt(d2[:, 0] * d2[:, 0] + d2[:, 1] * d2[:, 1] + d2[:, 2] * d2[:, 2])
    with np.errstate(invalid="ignore", divide="ignore"):
        c = d1[:, 0] * d2[:, 0] + d1[:, 1] * d2[:, 1] + d1[:, 2] * d2[:, 2]
        c = c / (g.r1 * g.r2)
    g.c = np.minimum(np.maximum(c, -1.0), 1.0)
    return g


def _terms(T, g, bonds, angles, p):
    """the term records in the number type T (np.longdouble: the reference; np.float64: the restatement) -> bond and angle
    namespaces with the forces on the members, the energy, the six virial products and (longdouble only) their magnitudes"""
    bk, br = np.concatenate([[0.0], p.bond_k]).astype(T), np.concatenate([[0.0], p.bond_r0]).astype(T)
    ak, a0 = np.concatenate([[0.0], p.angle_k]).astype(T), np.concatenate([[0.0], p.angle_theta0]).astype(T)
    B, A = SimpleNamespace(), SimpleNamespace()
    # bonds
    t = bonds[:, 2]
    d = g.bx1.astype(T) - g.bx2.astype(T)
    r = g.r.astype(T)
    dr = r - br[t]
    rk = bk[t] * dr
    pos = r > 0
    rs = np.where(pos, r, T(1))
    fb = np.where(pos, -2 * rk / rs, T(0))
    B.e = rk * dr
    B.f1 = d * fb[:, None]
    B.v = _six(d, d) * fb[:, None]
    drm = r + np.abs(br[t])
    rkm = np.abs(bk[t]) * drm
    fbm = np.where(pos, 2 * rkm / rs, T(0))
    B.e_abs = rkm * drm
    B.f1_abs = np.abs(d) * fbm[:, None]
    B.v_abs = np.abs(_six(d, d)) * fbm[:, None]
    # angles
    t = angles[:, 3]
    d1, d2 = g.a1.astype(T) - g.ac.astype(T), g.a3.astype(T) - g.ac.astype(T)
    rsq1 = d1[:, 0] * d1[:, 0] + d1[:, 1] * d1[:, 1] + d1[:, 2] * d1[:, 2]
    rsq2 = d2[:, 0] * d2[:, 0] + d2[:, 1] * d2[:, 1] + d2[:, 2] * d2[:, 2]
    r1, r2, c = g.r1.astype(T), g.r2.astype(T), g.c.astype(T)
    s = np.sqrt(1 - c * c)
    s = 1 / np.where(s < T(0.001), T(0.001), s)
    ac = np.arccos(c)
    dth = ac - a0[t]
    tk = ak[t] * dth
    A.e = tk * dth
    a = -2 * tk * s
    a11, a12, a22 = a * c / rsq1, -a / (r1 * r2), a * c / rsq2
    A.f1 = a11[:, None] * d1 + a12[:, None] * d2
    A.f3 = a22[:, None] * d2 + a12[:, None] * d1
    A.v = _six(d1, A.f1) + _six(d2, A.f3)
    dthm = ac + np.abs(a0[t])
    tkm = np.abs(ak[t]) * dthm
    A.e_abs = tkm * dthm
    am = 2 * tkm * s
    a11m, a12m, a22m = am * np.abs(c) / rsq1, am / (r1 * r2), am * np.abs(c) / rsq2
    A.f1_abs = a11m[:, None] * np.abs(d1) + a12m[:, None] * np.abs(d2)
    A.f3_abs = a22m[:, None] * np.abs(d2) + a12m[:, None] * np.abs(d1)
    A.v_abs = _six(np.abs(d1), A.f1_abs) + _six(np.abs(d2), A.f3_abs)
    return B, A


def _gather(T, nall, nlocal, newton, bonds, angles, B, A, mag):
    """the per-atom sums, contributions added one at a time in slot order (np.add.at): bonds first in list order, then angles"""
    sfx = "_abs" if mag else ""
    sign = 1 if mag else -1
    nb, na = len(bonds), len(angles)
    idx = np.concatenate([bonds[:, :2].reshape(-1), angles[:, :3].reshape(-1)])
    bf = getattr(B, "f1" + sfx)
    af1, af3 = getattr(A, "f1" + sfx), getattr(A, "f3" + sfx)
    mid = af1 + af3
    fv = np.concatenate([np.stack([bf, sign * bf], 1).reshape(-1, 3), np.stack([af1, sign * mid, af3], 1).reshape(-1, 3)])
    be, ae = getattr(B, "e" + sfx) * T(0.5), getattr(A, "e" + sfx) * T(THIRD)
    ev = np.concatenate([np.repeat(be, 2), np.repeat(ae, 3)])
    bv, av = getattr(B, "v" + sfx) * T(0.5), getattr(A, "v" + sfx) * T(THIRD)
    vv = np.concatenate([np.repeat(bv, 2, axis=0), np.repeat(av, 3, axis=0)])
    keep = np.full(len(idx), True) if newton else idx < nlocal
    f, ea, va = np.zeros((nall, 3), dtype=T), np.zeros(nall, dtype=T), np.zeros((nall, 6), dtype=T)
    np.add.at(f, idx[keep], fv[keep])
    np.add.at(ea, idx[keep], ev[keep])
    np.add.at(va, idx[keep], vv[keep])
    # the term's weight in the global tallies
    if newton:
        wb, wa = np.ones(nb, dtype=T), np.ones(na, dtype=T)
    else:
        wb = T(0.5) * (bonds[:, :2] < nlocal).sum(axis=1)
        wa = T(THIRD) * (angles[:, :3] < nlocal).sum(axis=1)
    eng = np.array([(wb * getattr(B, "e" + sfx)).sum(), (wa * getattr(A, "e" + sfx)).sum()], dtype=T)
    W = (wb[:, None] * getattr(B, "v" + sfx)).sum(axis=0) + (wa[:, None] * getattr(A, "v" + sfx)).sum(axis=0)
    return f, eng, W, ea, va


def _run(T, x, nlocal, bonds, angles, p, newton, prd):
    bonds, angles = _lists(bonds, angles)
    nall = len(x)
    g = _geometry(x, bonds, angles, prd)
    with np.errstate(invalid="ignore", divide="ignore"):
        B, A = _terms(T, g, bonds, angles, p)
        f, eng, W, ea, va = _gather(T, nall, nlocal, newton, bonds, angles, B, A, False)
        R = SimpleNamespace(f=f, eng=eng, W=W, eatom=ea, vatom=va, geom=g, B=B, Ang=A, bonds=bonds, angles=angles)
        R.A, R.E_abs, R.W_abs, R.eatom_abs, R.vatom_abs = _gather(T, nall, nlocal, newton, bonds, angles, B, A, True)
    return R


def reference(x, nlocal, bonds, angles, p, newton, prd=(0.0, 0.0, 0.0)):
    return _run(LD, x, nlocal, bonds, angles, p, newton, prd)


def restate64(x, nlocal, bonds, angles, p, newton, prd=(0.0, 0.0, 0.0)):
    """the kernels' arithmetic in float64 numpy: -> (f, eng, W, eatom, vatom)"""
    R = _run(np.float64, x, nlocal, bonds, angles, p, newton, prd)
    return R.f, R.eng, R.W, R.eatom, R.vatom


def for_case(c):
    return reference(c.x, c.nlocal, c.bonds, c.angles, c.p, c.newton, c.prd)


def frac(tag, got, want, bound):
    """largest |got - want| / bound over the entries (0 / 0 counts as 0: an entry without terms must be exact)"""
    err = np.abs(np.asarray(got, dtype=LD) - want)
    bound = np.asarray(bound, dtype=LD) * np.ones_like(err)
    assert np.all(err[bound == 0] == 0), tag
    fr = float((err[bound > 0] / bound[bound > 0]).max()) if np.any(bound > 0) else 0.0
    print(f"{tag}: {fr:.3g} of the bound")
    return fr


def check(tag, got, R, slack=None):
    """(f, eng, W, eatom, vatom) of an entry against the reference, entry-wise to TOL of the magnitude; None entries are skipped.
    slack: what the rounding of a pre-filled f adds (None: f started as zeros) -> the fractions of the bound"""
    f, eng, W, ea, va = got
    fr = {}
    if f is not None:
        fr["f"] = frac(f"{tag}: force", f, R.f, TOL * R.A + (0 if slack is None else slack))
    if eng is not None:
        fr["eng"] = frac(f"{tag}: ebond, eangle", eng, R.eng, TOL * R.E_abs)
    if W is not None:
        fr["W"] = frac(f"{tag}: virial", W, R.W, TOL * R.W_abs)
    if ea is not None:
        fr["eatom"] = frac(f"{tag}: eatom", ea, R.eatom, TOL * R.eatom_abs)
    if va is not None:
        fr["vatom"] = frac(f"{tag}: vatom", va, R.vatom, TOL * R.vatom_abs)
    assert max(fr.values()) <= 1.0, (tag, fr)
    return fr


def fold(v, owner, nlocal):
    """ghost entries added onto their owners: what LAMMPS' reverse communication does (one rank, periodic images)"""
    out = np.zeros((nlocal,) + v.shape[1:], dtype=v.dtype)
    np.add.at(out, owner, v)
    return out


# ---- input builders ---------------------------------------------------------------------------------------------------------------
def bent(rng, centre, lo_deg=30.0, hi_deg=150.0):
    """the two outer atoms of bent molecules around `centre` [n][3]: bond lengths 0.9-1.4, angles lo_deg-hi_deg, random orientation"""
    n = len(centre)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    w = np.cross(u, rng.normal(size=(n, 3))); w /= np.linalg.norm(w, axis=1)[:, None]
    th = np.deg2rad(rng.uniform(lo_deg, hi_deg, n))[:, None]
    r1, r2 = rng.uniform(0.9, 1.4, (n, 1)), rng.uniform(0.9, 1.4, (n, 1))
    return centre + r1 * u, centre + r2 * (np.cos(th) * u + np.sin(th) * w)


def _case(tag, x, nlocal, bonds, angles, newton=True, prd=(0.0, 0.0, 0.0), p=PARAMS, **kw):
    bonds, angles = _lists(bonds, angles)
    return SimpleNamespace(tag=tag, x=np.ascontiguousarray(x, dtype=np.float64), nlocal=int(nlocal), nall=len(x),
                           bonds=bonds.astype(np.int32), angles=angles.astype(np.int32), newton=bool(newton),
                           prd=tuple(float(v) for v in prd), p=p, **kw)


def molecule_system(seed=11):
    """systems.small_random(ne_side=4, n_elyte=64) with its electrolyte atoms taken three at a time as bent molecules: the middle
    atom of a triple stays, the two others are placed around it and wrapped into the box.  Seven molecules are moved to the
    periodic faces and to one edge first.  -> (system, bonds, angles) with owned indices; one electrolyte atom and every electrode
    atom are in no term"""
    import dataclasses
    from conp_amd import systems
    s = systems.small_random(ne_side=4, n_elyte=64)
    el = np.nonzero(s.echeck == 0)[0]
    assert len(el) == 64
    mol = el[:63].reshape(21, 3)
    rng = np.random.default_rng(seed)
    x = s.x.copy()
    lo, hi, prd = s.boxlo, s.boxhi, s.prd
    cen = x[mol[:, 1]].copy()
    per = [c for c in range(3) if s.periodic[c]]
    k, faces = 0, []
    for c in per:                                     # a molecule on the lower and one on the upper side of every periodic face
        cen[k, c] = lo[c] + 0.05; cen[k + 1, c] = hi[c] - 0.05
        faces += [(k, c, -1.0), (k + 1, c, 1.0)]
        k += 2
    cen[k, 0] = lo[0] + 0.05; cen[k, 1] = hi[1] - 0.05          # one on an edge
    faces += [(k, 0, -1.0), (k, 1, 1.0)]
    x[mol[:, 1]] = cen
    p1, p3 = bent(rng, cen)
    for m, c, sign in faces:                          # mirrored as a whole, so that its first atom lies beyond the face
        if (p1[m, c] - cen[m, c]) * sign < 0:
            p1[m, c], p3[m, c] = 2 * cen[m, c] - p1[m, c], 2 * cen[m, c] - p3[m, c]
    x[mol[:, 0]], x[mol[:, 2]] = p1, p3
    for c in per:                                     # the wrap of LAMMPS' remap: into [lo, hi)
        x[:, c] = np.where(x[:, c] < lo[c], x[:, c] + prd[c], x[:, c])
        x[:, c] = np.where(x[:, c] >= hi[c], x[:, c] - prd[c], x[:, c])
    bt = rng.integers(1, 4, (21, 2))
    bonds = np.stack([np.stack([mol[:, 1], mol[:, 0], bt[:, 0]], 1), np.stack([mol[:, 1], mol[:, 2], bt[:, 1]], 1)], 1).reshape(-1, 3)
    angles = np.stack([mol[:, 0], mol[:, 1], mol[:, 2], rng.integers(1, 3, 21)], 1)
    return dataclasses.replace(s, x=np.ascontiguousarray(x)), bonds, angles


def molecules(newton, form):
    """case 1.  form "image": owned indices and prd of the box;  form "ghost": ghosts from neighbor.make_ghosts, every partner
    replaced by the ghost (or owned atom) that carries the closest image's coordinates bit for bit, prd = 0 -- plus one bond and one
    angle between ghosts only (with newton off: weights 0, no force)"""
    from conp_amd import neighbor
    s, bonds, angles = molecule_system()
    prd = np.where(s.periodic, s.prd, 0.0)
    if form == "image":
        c = _case(f"molecules, closest image, newton {newton}", s.x, s.natoms, bonds, angles, newton, prd)
        c.s, c.owner = s, np.arange(s.natoms)
        return c
    at = neighbor.make_ghosts(s)
    key = {(int(o), at.x[i].tobytes()): i for i, o in enumerate(at.owner)}
    shift_of = np.rint((at.x - at.x[at.owner]) / np.where(prd > 0, prd, 1.0)).astype(np.int64)
    by_shift = {(int(o), tuple(sh)): i for i, (o, sh) in enumerate(zip(at.owner, shift_of))}

    def image_index(anchor, partner):
        xi, _ = closest_image(at.x[anchor], at.x[partner], prd)
        return np.array([key[(int(pp), v.tobytes())] for pp, v in zip(partner, xi)])
    gb, ga = bonds.copy(), angles.copy()
    gb[:, 1] = image_index(bonds[:, 0], bonds[:, 1])
    ga[:, 0] = image_index(angles[:, 1], angles[:, 0])
    ga[:, 2] = image_index(angles[:, 1], angles[:, 2])
    # a whole molecule among the ghosts: the first molecule all of whose atoms have an image under one shift
    extra = None
    for m in range(len(angles)):
        for sh in sorted({tuple(int(k) for k in v) for v in shift_of[at.nlocal:]}):
            idx = [by_shift.get((int(a), sh)) for a in angles[m, :3]]
            if None not in idx and extra is None:
                extra = (m, idx)
    assert extra is not None
    m, idx = extra
    gb = np.concatenate([gb, [[idx[1], idx[0], bonds[2 * m, 2]]]])
    ga = np.concatenate([ga, [[idx[0], idx[1], idx[2], angles[m, 3]]]])
    c = _case(f"molecules, ghost indices, newton {newton}", at.x, at.nlocal, gb, ga, newton)
    c.s, c.owner, c.at = s, at.owner, at
    return c


def hub(n=70, seed=3):
    """case 2: atom 0 is the centre of n angles and a member of n bonds: more slots than a wavefront has lanes, a ragged tail"""
    rng = np.random.default_rng(seed)
    x = np.zeros((n + 4, 3))
    x[0] = (5.0, 6.0, 7.0)
    u = rng.normal(size=(n + 1, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    x[1:n + 2] = x[0] + rng.uniform(0.9, 1.4, (n + 1, 1)) * u
    x[n + 2:] = rng.uniform(0, 10, (2, 3))                            # two atoms in no term
    k = np.arange(1, n + 1)
    bonds = np.stack([np.zeros(n, int), k, rng.integers(1, 4, n)], 1)
    angles = np.stack([k, np.zeros(n, int), k + 1, rng.integers(1, 3, n)], 1)
    return _case(f"hub of {n}", x, len(x), bonds, angles)


def edges(nbond, nangle, natoms=None, seed=5, newton=True):
    """case 3: the first nbond bonds and the first nangle angles of bent molecules (30-150 degrees) over randomly numbered atoms;
    natoms: the atom count (at least 3 per molecule and two more; the rest is in no term); with newton off the last tenth of the
    atoms are ghosts"""
    rng = np.random.default_rng(seed)
    nmol = max((nbond + 1) // 2, nangle, 1)
    natoms = max(natoms or 0, 3 * nmol + 2)
    perm = rng.permutation(natoms)
    k = int(np.nonzero(perm == natoms - 1)[0][0])
    perm[0], perm[k] = perm[k], perm[0]                      # the last atom is in the first bond and the first angle
    mol = perm[:3 * nmol].reshape(nmol, 3)
    x = rng.uniform(0.0, 40.0, (natoms, 3))
    x[mol[:, 0]], x[mol[:, 2]] = bent(rng, x[mol[:, 1]])
    bt = rng.integers(1, 4, (nmol, 2))
    bonds = np.stack([np.stack([mol[:, 1], mol[:, 0], bt[:, 0]], 1), np.stack([mol[:, 1], mol[:, 2], bt[:, 1]], 1)], 1).reshape(-1, 3)
    angles = np.stack([mol[:, 0], mol[:, 1], mol[:, 2], rng.integers(1, 3, nmol)], 1)
    nlocal = natoms if newton else natoms - natoms // 10
    return _case(f"{nbond} bonds, {nangle} angles, {natoms} atoms, newton {newton}", x, nlocal, bonds[:nbond], angles[:nangle], newton)


# (nbond, nangle, natoms): 255 / 256 / 257 terms of either kind alone; one more atom than a workgroup of the gather kernel holds,
# the last atom in a term; one more term than a workgroup of the term kernel holds, bonds and angles mixed, with one more atom than
# two workgroups hold; one more term than BLOCK * FINISH (a finishing thread's second row) with one more atom than 257 workgroups hold
EDGE_SHAPES = [(BLOCK - 1, 0, None), (BLOCK, 0, None), (BLOCK + 1, 0, None), (0, BLOCK - 1, None), (0, BLOCK, None),
               (0, BLOCK + 1, None), (170, 85, BLOCK + 1), (172, 85, 2 * BLOCK + 1), (43692, 21845, 257 * BLOCK + 1)]
assert sum(EDGE_SHAPES[7][:2]) == BLOCK + 1 and sum(EDGE_SHAPES[8][:2]) == BLOCK * FINISH + 1


def degenerate():
    """case 4: a bond of length exactly 0; collinear triples on an axis with coordinates that are multiples of 0.5 (c = -1 and
    c = +1 exactly: s = 1000); a triple at 179.97 degrees (the 0.001 clamp is active, sqrt(1 - c^2) about 5e-4); a bond within
    1e-9 of r0; an angle within 1e-9 rad of theta0"""
    p = PARAMS
    th = np.deg2rad(179.97)
    t0 = p.angle_theta0[0] + 5e-10
    x = np.array([
        [3.0, 4.0, 5.0], [3.0, 4.0, 5.0],                                            # 0, 1: the bond of length 0
        [10.0, 2.0, 2.0], [10.5, 2.0, 2.0], [11.5, 2.0, 2.0],                        # 2-4: collinear, centre 3: c = -1
        [2.0, 11.0, 3.0], [2.0, 11.5, 3.0], [2.0, 13.0, 3.0],                        # 5-7: collinear, centre 5: c = +1
        [20.0, 20.0, 20.0], [21.0, 20.0, 20.0], [20.0 + 1.2 * np.cos(th), 20.0 + 1.2 * np.sin(th), 20.0],      # 8-10, centre 8
        [30.0, 1.0, 1.0], [30.0 + p.bond_r0[1] + 5e-10, 1.0, 1.0],                   # 11, 12: r within 1e-9 of r0 of type 2
        [1.0, 30.0, 1.0], [2.0, 30.0, 1.0], [1.0 + 1.1 * np.cos(t0), 30.0, 1.0 + 1.1 * np.sin(t0)],            # 13-15, centre 13
        [15.0, 15.0, 15.0]])                                                         # 16: in no term
    bonds = [[0, 1, 1], [11, 12, 2], [3, 2, 3], [3, 4, 1]]
    angles = [[2, 3, 4, 1], [6, 5, 7, 2], [9, 8, 10, 1], [14, 13, 15, 1]]
    return _case("degenerate terms", x, len(x), bonds, angles)


def gpu_cases():
    """every input the GPU tests use (tests/test_bonded_ref_math.py holds the float64 restatement to the bound on each)"""
    out = [molecules(n, f) for f in ("ghost", "image") for n in (True, False)]
    out.append(hub())
    out += [edges(*e) for e in EDGE_SHAPES]
    out.append(edges(172, 85, 2 * BLOCK + 1, newton=False))
    out.append(degenerate())
    return out


def conditioning(R):
    """the smallest sqrt(1 - c^2) over the angles whose c is not exactly +-1 (the condition of the bound: at least 2e-4)"""
    c = R.geom.c
    free = np.abs(c) != 1.0
    return float(np.sqrt(1 - c[free].astype(LD) ** 2).min()) if free.any() else np.inf
