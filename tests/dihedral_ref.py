"""numpy reference (np.longdouble) of the opls / harmonic dihedrals and the harmonic / cvff impropers, straight from the definition in
include/conp_hip.h (conp_dihedral_compute).

One thing is part of the definition: the closest images are float64 as written (they are coordinates a ghost would carry).
Everything downstream of the four member positions is longdouble.

reference(...) returns the results (f, eng, W, eatom, vatom) and the cancellation-free magnitudes the bounds of the GPU tests are
stated against -- every term replaced by its absolute value and every difference by the sum of its operands' magnitudes:
A[nall][3], E_abs[2], W_abs[6], eatom_abs[nall], vatom_abs[nall][6].  Three choices in them:
  - F, G, H count with their own absolute values (a difference of coordinates a bond length apart loses nothing that the offset of
    the coordinates does not already bound, and the reference forms them from the same float64 images);
  - sin(k phi) and cos(k phi) count as 1: their rounding follows the ABSOLUTE error of k phi, not their value (sin(pi) of a float64
    pi is 1.2e-16, not 0), so |K sin(k phi)| would promise an accuracy no float64 evaluation has near phi = 0 and phi = pi;
  - |phi| - chi0 counts as |phi| + |chi0|.
The divisions by A2, B2 and g are kept as they are: their relative rounding grows with 1 / sin^2 of the two bond angles, which is
why the inputs keep those sines at 0.25 or more (conditioning(), tests/test_dihedral_ref_math.py).
restate64(...) is the same arithmetic in float64 in the kernels' order; the builders below make the inputs of the GPU tests."""
from types import SimpleNamespace

import numpy as np

from bonded_ref import closest_image, fold, frac  # noqa: F401  (the image rule and the bound's bookkeeping are section 21's)

LD = np.longdouble
TOL = 1e-12       # the bound of tests/bonded_ref.py
# launch shapes of conp_dihedral.hip, restated (tests/test_dihedral_ref_math.py compares them with csrc/conp_kernels.h)
BLOCK = 256       # threads of a workgroup: one term each (term kernel), one atom each (gather kernel)
FINISH = 256      # threads of the finishing workgroup: from BLOCK * FINISH terms on a thread adds a second row
TERM_W = 16
OPLS, COSINE, QUADRATIC = 0, 1, 2                       # the three energy functions of the four styles
FORM = {("dihedral", "opls"): OPLS, ("dihedral", "harmonic"): COSINE, ("improper", "harmonic"): QUADRATIC, ("improper", "cvff"): COSINE}

# the two style pairs of the GPU tests: dihedral_coeff / improper_coeff rows as the deck gives them (chi0 in radians at the ABI)
PARAMS_OPLS = SimpleNamespace(dstyle="opls", dcoef=np.array([[1.3, -0.05, 0.2, 0.0], [0.0, 7.25, 0.0, 0.0], [-1.5, 0.8, 2.9, -0.4]]),
                              istyle="harmonic", icoef=np.array([[2.1, np.deg2rad(35.26)], [15.0, 0.0]]))
PARAMS_COS = SimpleNamespace(dstyle="harmonic", dcoef=np.array([[1.2, 1.0, 3.0], [0.7, -1.0, 0.0], [2.0, -1.0, 2.0]]),
                             istyle="cvff", icoef=np.array([[1.1, -1.0, 2.0], [0.5, 1.0, 3.0]]))
PAIRS = {"opls": PARAMS_OPLS, "cos": PARAMS_COS}


def _lists(dihedrals, impropers):
    d = np.asarray(dihedrals if dihedrals is not None else np.zeros((0, 5)), dtype=np.int64).reshape(-1, 5)
    i = np.asarray(impropers if impropers is not None else np.zeros((0, 5)), dtype=np.int64).reshape(-1, 5)
    return d, i


def _six(u, v):
    """(ux vx, uy vy, uz vz, ux vy, ux vz, uy vz)"""
    return np.stack([u[:, 0] * v[:, 0], u[:, 1] * v[:, 1], u[:, 2] * v[:, 2], u[:, 0] * v[:, 1], u[:, 0] * v[:, 2], u[:, 1] * v[:, 2]], 1)


def _cross(u, v):
    return np.stack([u[:, 1] * v[:, 2] - u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] - u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] - u[:, 1] * v[:, 0]], 1)


def _cross_abs(u, v):
    u, v = np.abs(u), np.abs(v)
    return np.stack([u[:, 1] * v[:, 2] + u[:, 2] * v[:, 1], u[:, 2] * v[:, 0] + u[:, 0] * v[:, 2], u[:, 0] * v[:, 1] + u[:, 1] * v[:, 0]], 1)


def _dot(u, v):
    return u[:, 0] * v[:, 0] + u[:, 1] * v[:, 1] + u[:, 2] * v[:, 2]


def _geometry(x, terms, prd):
    """the float64 part of the definition: x1' and x3' seen from x2, x4' seen from x3' -> positions and shifts"""
    x = np.asarray(x, dtype=np.float64)
    g = SimpleNamespace()
    g.p2 = x[terms[:, 1]]
    g.p1, g.s1 = closest_image(g.p2, x[terms[:, 0]], prd)
    g.p3, g.s3 = closest_image(g.p2, x[terms[:, 2]], prd)
    g.p4, g.s4 = closest_image(g.p3, x[terms[:, 3]], prd)
    return g


def table(p):
    """-> (rows [ndihedraltypes + 1][4], rows [nimpropertypes + 1][4]) as the ABI takes them"""
    def tab(rows):
        r = np.asarray(rows, dtype=np.float64).reshape(len(rows), -1) if len(rows) else np.zeros((0, 4))
        t = np.zeros((len(r) + 1, 4))
        t[1:, :r.shape[1]] = r
        return t
    return tab(p.dcoef), tab(p.icoef)


def energy(T, form, k, phi):
    """e(phi), de(phi) and their magnitudes, per term; form [n], k [n][4]"""
    K1, K2, K3, K4 = (k[:, c] for c in range(4))
    one = T(1)
    eo = T(0.5) * (K1 * (one + np.cos(phi)) + K2 * (one - np.cos(T(2) * phi)) + K3 * (one + np.cos(T(3) * phi)) + K4 * (one - np.cos(T(4) * phi)))
    do = T(0.5) * (T(2) * (K2 * np.sin(T(2) * phi)) - K1 * np.sin(phi) - T(3) * (K3 * np.sin(T(3) * phi)) + T(4) * (K4 * np.sin(T(4) * phi)))
    a1, a2, a3, a4 = (np.abs(v) for v in (K1, K2, K3, K4))
    eo_abs, do_abs = a1 + a2 + a3 + a4, T(0.5) * (a1 + T(2) * a2 + T(3) * a3 + T(4) * a4)
    an = K3 * phi                                       # cosine rows: K d n
    ec = K1 * (one + K2 * np.cos(an))
    dc = -(K1 * K2 * K3 * np.sin(an))
    ec_abs, dc_abs = T(2) * a1, a1 * a3
    u = np.abs(phi) - K2                                # quadratic rows: K chi0
    eq = K1 * u * u
    dq = T(2) * K1 * (phi - np.copysign(K2, phi))
    um = np.abs(phi) + a2
    eq_abs, dq_abs = a1 * um * um, T(2) * a1 * um
    pick = lambda o, c, q: np.where(form == OPLS, o, np.where(form == COSINE, c, q))
    return pick(eo, ec, eq), pick(do, dc, dq), pick(eo_abs, ec_abs, eq_abs), pick(do_abs, dc_abs, dq_abs)


def terms_of(T, p1, p2, p3, p4, form, k):
    """the term records in the number type T from the four member positions (images already taken) -> a namespace with phi, the
    forces on the members, the energy, the six virial products and their magnitudes; a degenerate term is all zeros"""
    p1, p2, p3, p4, k = (np.asarray(v).astype(T) for v in (p1, p2, p3, p4, k))
    R = SimpleNamespace()
    F, G, H = p1 - p2, p2 - p3, p4 - p3
    A, B = _cross(F, G), _cross(H, G)
    Am, Bm = _cross_abs(F, G), _cross_abs(H, G)
    A2, B2, g = _dot(A, A), _dot(B, B), np.sqrt(_dot(G, G))
    ok = (A2 != 0) & (B2 != 0) & (g != 0)
    A2s, B2s, gs = np.where(ok, A2, T(1)), np.where(ok, B2, T(1)), np.where(ok, g, T(1))
    C = _cross(B, A)
    R.phi = np.arctan2(_dot(C, G) / gs, _dot(A, B))
    e, de, e_abs, de_abs = energy(T, form, k, R.phi)
    p = -de
    ga, gb = (gs / A2s)[:, None], (gs / B2s)[:, None]
    sa, sb = (_dot(F, G) / (A2s * gs))[:, None], (_dot(H, G) / (B2s * gs))[:, None]
    sam, sbm = (_dot(np.abs(F), np.abs(G)) / (A2s * gs))[:, None], (_dot(np.abs(H), np.abs(G)) / (B2s * gs))[:, None]
    d1, d4, s = -(ga * A), gb * B, sa * A - sb * B
    d3 = (-d4) - s
    d1m, d4m, sm = ga * Am, gb * Bm, sam * Am + sbm * Bm
    d3m = d4m + sm
    z = ok[:, None]
    R.f1, R.f3, R.f4 = (np.where(z, p[:, None] * d, T(0)) for d in (d1, d3, d4))
    R.f2 = -((R.f1 + R.f3) + R.f4)
    R.f1_abs, R.f3_abs, R.f4_abs = (np.where(z, de_abs[:, None] * d, T(0)) for d in (d1m, d3m, d4m))
    R.f2_abs = (R.f1_abs + R.f3_abs) + R.f4_abs
    R.e, R.e_abs = np.where(ok, e, T(0)), np.where(ok, e_abs, T(0))
    R.v = _six(F, R.f1) + _six(-G, R.f3) + _six(H - G, R.f4)
    R.v_abs = _six(np.abs(F), R.f1_abs) + _six(np.abs(G), R.f3_abs) + _six(np.abs(H) + np.abs(G), R.f4_abs)
    R.ok, R.F, R.G, R.H = ok, F, G, H
    with np.errstate(invalid="ignore", divide="ignore"):
        R.sin1, R.sin2 = np.sqrt(A2 / (_dot(F, F) * g * g)), np.sqrt(B2 / (_dot(H, H) * g * g))       # the two bond-angle sines
    return R


def _gather(T, nall, nlocal, newton, terms, nd, R, mag):
    """the per-atom sums, contributions added one at a time in slot order (np.add.at): dihedrals first in list order, then
    impropers, the roles of a term in member order"""
    sfx = "_abs" if mag else ""
    get = lambda n: getattr(R, n + sfx)
    idx = terms[:, :4].reshape(-1)
    fv = np.stack([get("f1"), get("f2"), get("f3"), get("f4")], 1).reshape(-1, 3)
    ev = np.repeat(get("e") * T(0.25), 4)
    vv = np.repeat(get("v") * T(0.25), 4, axis=0)
    keep = np.full(len(idx), True) if newton else idx < nlocal
    f, ea, va = np.zeros((nall, 3), dtype=T), np.zeros(nall, dtype=T), np.zeros((nall, 6), dtype=T)
    np.add.at(f, idx[keep], fv[keep])
    np.add.at(ea, idx[keep], ev[keep])
    np.add.at(va, idx[keep], vv[keep])
    w = np.ones(len(terms), dtype=T) if newton else T(0.25) * (terms[:, :4] < nlocal).sum(axis=1)      # the weight in the global tallies
    we = w * get("e")
    eng = np.array([we[:nd].sum(), we[nd:].sum()], dtype=T)
    W = (w[:, None] * get("v")).sum(axis=0)
    return f, eng, W, ea, va


def forms_and_rows(p, dihedrals, impropers):
    dt, it = table(p)
    form = np.concatenate([np.full(len(dihedrals), FORM[("dihedral", p.dstyle)] if len(dihedrals) else 0),
                           np.full(len(impropers), FORM[("improper", p.istyle)] if len(impropers) else 0)]).astype(np.int64)
    k = np.concatenate([dt[dihedrals[:, 4]], it[impropers[:, 4]]])
    return form, k


def _run(T, x, nlocal, dihedrals, impropers, p, newton, prd):
    dihedrals, impropers = _lists(dihedrals, impropers)
    terms = np.concatenate([dihedrals, impropers])
    nall, nd = len(x), len(dihedrals)
    g = _geometry(x, terms, prd)
    form, k = forms_and_rows(p, dihedrals, impropers)
    with np.errstate(invalid="ignore", divide="ignore"):
        t = terms_of(T, g.p1, g.p2, g.p3, g.p4, form, k)
        f, eng, W, ea, va = _gather(T, nall, nlocal, newton, terms, nd, t, False)
        R = SimpleNamespace(f=f, eng=eng, W=W, eatom=ea, vatom=va, geom=g, T=t, terms=terms, nd=nd, form=form, k=k)
        R.A, R.E_abs, R.W_abs, R.eatom_abs, R.vatom_abs = _gather(T, nall, nlocal, newton, terms, nd, t, True)
    return R


def reference(x, nlocal, dihedrals, impropers, p, newton, prd=(0.0, 0.0, 0.0)):
    return _run(LD, x, nlocal, dihedrals, impropers, p, newton, prd)


def restate64(x, nlocal, dihedrals, impropers, p, newton, prd=(0.0, 0.0, 0.0)):
    """the kernels' arithmetic in float64 numpy: -> (f, eng, W, eatom, vatom)"""
    R = _run(np.float64, x, nlocal, dihedrals, impropers, p, newton, prd)
    return R.f, R.eng, R.W, R.eatom, R.vatom


def for_case(c):
    return reference(c.x, c.nlocal, c.dihedrals, c.impropers, c.p, c.newton, c.prd)


def check(tag, got, R, slack=None, tol=TOL):
    """(f, eng, W, eatom, vatom) of an entry against the reference, entry-wise to tol of the magnitude; None entries are skipped.
    slack: what the rounding of a pre-filled f adds (None: f started as zeros) -> the fractions of the bound"""
    f, eng, W, ea, va = got
    fr = {}
    if f is not None:
        fr["f"] = frac(f"{tag}: force", f, R.f, tol * R.A + (0 if slack is None else slack))
    if eng is not None:
        fr["eng"] = frac(f"{tag}: edihedral, eimproper", eng, R.eng, tol * R.E_abs)
    if W is not None:
        fr["W"] = frac(f"{tag}: virial", W, R.W, tol * R.W_abs)
    if ea is not None:
        fr["eatom"] = frac(f"{tag}: eatom", ea, R.eatom, tol * R.eatom_abs)
    if va is not None:
        fr["vatom"] = frac(f"{tag}: vatom", va, R.vatom, tol * R.vatom_abs)
    assert max(fr.values()) <= 1.0, (tag, fr)
    return fr


def conditioning(R):
    """the smallest bond-angle sine over the terms that are not degenerate (the condition of the bound: at least 0.25)"""
    ok = R.T.ok
    return float(min(R.T.sin1[ok].min(), R.T.sin2[ok].min())) if ok.any() else np.inf


# ---- input builders ---------------------------------------------------------------------------------------------------------------
def _unit(v):
    return v / np.linalg.norm(v, axis=1)[:, None]


def chain(rng, n, lo_deg=30.0, hi_deg=150.0):
    """n four-atom chains around the origin -> [n][4][3]: bond lengths 0.9-1.6, the two bond angles lo_deg-hi_deg (sines of 0.5 or
    more at the defaults), the torsion uniform in (-pi, pi), random orientation"""
    u = _unit(rng.normal(size=(n, 3)))                                  # from member 2 to member 3
    e1 = _unit(np.cross(u, rng.normal(size=(n, 3))))
    e2 = np.cross(u, e1)
    r1, r2, r3 = (rng.uniform(0.9, 1.6, (n, 1)) for _ in range(3))
    t1, t2 = (np.deg2rad(rng.uniform(lo_deg, hi_deg, (n, 1))) for _ in range(2))
    ph = rng.uniform(-np.pi, np.pi, (n, 1))
    p2 = np.zeros((n, 3))
    p3 = r2 * u
    p1 = r1 * (np.cos(t1) * u + np.sin(t1) * e1)
    p4 = p3 + r3 * (-np.cos(t2) * u + np.sin(t2) * (np.cos(ph) * e1 + np.sin(ph) * e2))
    return np.stack([p1, p2, p3, p4], 1)


def _case(tag, x, nlocal, dihedrals, impropers, newton=True, prd=(0.0, 0.0, 0.0), p=PARAMS_OPLS, **kw):
    dihedrals, impropers = _lists(dihedrals, impropers)
    return SimpleNamespace(tag=tag, x=np.ascontiguousarray(x, dtype=np.float64), nlocal=int(nlocal), nall=len(x),
                           dihedrals=dihedrals.astype(np.int32), impropers=impropers.astype(np.int32), newton=bool(newton),
                           prd=tuple(float(v) for v in prd), p=p, **kw)


def molecule_system(seed=13):
    """systems.small_random(ne_side=4, n_elyte=64) with 60 of its electrolyte atoms taken four at a time as chains: the second atom
    of a quadruple stays, the three others are placed around it and wrapped into the box.  Seven molecules are moved to the periodic
    faces and to one edge first.  Every molecule carries a dihedral (1, 2, 3, 4) and an improper over the same atoms in the
    opposite order.  -> (system, dihedrals, impropers) with owned indices; four electrolyte atoms and every electrode atom are in no
    term"""
    import dataclasses
    from conp_amd import systems
    s = systems.small_random(ne_side=4, n_elyte=64)
    el = np.nonzero(s.echeck == 0)[0]
    assert len(el) == 64
    mol = el[:60].reshape(15, 4)
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
    pos = chain(rng, 15) + cen[:, None, :]
    for m, c, sign in faces:                          # mirrored as a whole, so that its third and fourth atom lie beyond the face
        if (pos[m, 2, c] - cen[m, c]) * sign < 0:
            pos[m, :, c] = 2 * cen[m, c] - pos[m, :, c]
    x[mol.reshape(-1)] = pos.reshape(-1, 3)
    for c in per:                                     # the wrap of LAMMPS' remap: into [lo, hi)
        x[:, c] = np.where(x[:, c] < lo[c], x[:, c] + prd[c], x[:, c])
        x[:, c] = np.where(x[:, c] >= hi[c], x[:, c] - prd[c], x[:, c])
    dihedrals = np.concatenate([mol, rng.integers(1, 4, (15, 1))], 1)
    impropers = np.concatenate([mol[:, ::-1], rng.integers(1, 3, (15, 1))], 1)
    return dataclasses.replace(s, x=np.ascontiguousarray(x)), dihedrals, impropers


def molecules(pair, newton, form):
    """case 1.  pair: "opls" (opls with improper harmonic) or "cos" (harmonic with cvff).  form "image": owned indices and prd of the
    box;  form "ghost": ghosts from neighbor.make_ghosts, every member but the second replaced by the ghost (or owned atom) that
    carries the closest image's coordinates bit for bit, prd = 0 -- plus one dihedral and one improper between ghosts only (with
    newton off: weights 0, no force)"""
    from conp_amd import neighbor
    s, dihedrals, impropers = molecule_system()
    p = PAIRS[pair]
    prd = np.where(s.periodic, s.prd, 0.0)
    if form == "image":
        c = _case(f"molecules ({pair}), closest image, newton {newton}", s.x, s.natoms, dihedrals, impropers, newton, prd, p)
        c.s, c.owner = s, np.arange(s.natoms)
        return c
    at = neighbor.make_ghosts(s)
    key = {(int(o), at.x[i].tobytes()): i for i, o in enumerate(at.owner)}
    shift_of = np.rint((at.x - at.x[at.owner]) / np.where(prd > 0, prd, 1.0)).astype(np.int64)
    by_shift = {(int(o), tuple(sh)): i for i, (o, sh) in enumerate(zip(at.owner, shift_of))}

    def ghosted(terms):
        g = _geometry(at.x, terms, prd)
        out = terms.copy()
        for col, img in ((0, g.p1), (2, g.p3), (3, g.p4)):
            out[:, col] = [key[(int(pp), v.tobytes())] for pp, v in zip(terms[:, col], img)]
        return out
    gd, gi = ghosted(dihedrals), ghosted(impropers)
    # a whole molecule among the ghosts: the first molecule that crosses no face and all of whose atoms have an image under one shift
    extra = None
    go = _geometry(at.x, dihedrals, prd)
    whole = [m for m in range(len(dihedrals)) if not (go.s1[m].any() or go.s3[m].any() or go.s4[m].any())]
    for m in whole:
        for sh in sorted({tuple(int(k) for k in v) for v in shift_of[at.nlocal:]}):
            idx = [by_shift.get((int(a), sh)) for a in dihedrals[m, :4]]
            if None not in idx and extra is None:
                extra = (m, idx)
    assert extra is not None
    m, idx = extra
    gd = np.concatenate([gd, [idx + [dihedrals[m, 4]]]])
    gi = np.concatenate([gi, [idx[::-1] + [impropers[m, 4]]]])
    c = _case(f"molecules ({pair}), ghost indices, newton {newton}", at.x, at.nlocal, gd, gi, newton, p=p)
    c.s, c.owner, c.at = s, at.owner, at
    return c


def hub(n=70, seed=3):
    """case 2: atom 0 is a member of n terms, in role k % 4 of term k (40 dihedrals, then 30 impropers): more slots than a wavefront
    has lanes, a ragged tail, every role"""
    rng = np.random.default_rng(seed)
    pos = chain(rng, n)
    role = np.arange(n) % 4
    x0 = np.array([5.0, 6.0, 7.0])
    pos = pos - pos[np.arange(n), role][:, None, :] + x0              # the member of that role sits on atom 0
    x = np.zeros((1 + 3 * n + 2, 3))
    x[0] = x0
    terms = np.zeros((n, 5), dtype=np.int64)
    nxt = 1
    for k in range(n):
        for r in range(4):
            if r == role[k]:
                terms[k, r] = 0
            else:
                terms[k, r] = nxt; x[nxt] = pos[k, r]; nxt += 1
    x[nxt:] = rng.uniform(0, 10, (2, 3))                              # two atoms in no term
    nd = 40
    terms[:nd, 4] = rng.integers(1, 4, nd)
    terms[nd:, 4] = rng.integers(1, 3, n - nd)
    return _case(f"hub of {n}", x, len(x), terms[:nd], terms[nd:])


def edges(nd, ni, natoms=None, seed=5, newton=True, pair="opls"):
    """case 3: the first nd dihedrals and the first ni impropers of four-atom chains over randomly numbered atoms, coordinates up to
    40 A from the origin; natoms: the atom count (at least 4 per molecule and two more; the rest is in no term); with newton off the
    last tenth of the atoms are ghosts"""
    rng = np.random.default_rng(seed)
    nmol = max(nd, ni, 1)
    natoms = max(natoms or 0, 4 * nmol + 2)
    perm = rng.permutation(natoms)
    k = int(np.nonzero(perm == natoms - 1)[0][0])
    perm[0], perm[k] = perm[k], perm[0]                      # the last atom is in the first dihedral and the first improper
    mol = perm[:4 * nmol].reshape(nmol, 4)
    x = rng.uniform(0.0, 40.0, (natoms, 3))
    x[mol.reshape(-1)] = (chain(rng, nmol) + x[mol[:, 1]][:, None, :]).reshape(-1, 3)
    dihedrals = np.concatenate([mol, rng.integers(1, 4, (nmol, 1))], 1)
    impropers = np.concatenate([mol[:, ::-1], rng.integers(1, 3, (nmol, 1))], 1)
    nlocal = natoms if newton else natoms - natoms // 10
    return _case(f"{nd} dihedrals, {ni} impropers, {natoms} atoms, newton {newton}, {pair}", x, nlocal, dihedrals[:nd], impropers[:ni],
                 newton, p=PAIRS[pair])


# (ndihedral, nimproper, natoms, pair): 255 / 256 / 257 terms of either list alone; the same totals with the boundary between the
# lists inside a workgroup of the term kernel; one atom fewer and one more than a workgroup of the gather kernel holds, the last atom
# in a term; one more term than BLOCK * FINISH (a finishing thread's second row)
EDGE_SHAPES = [(BLOCK - 1, 0, None, "opls"), (BLOCK, 0, None, "cos"), (BLOCK + 1, 0, None, "opls"),
               (0, BLOCK - 1, None, "cos"), (0, BLOCK, None, "opls"), (0, BLOCK + 1, None, "cos"),
               (128, BLOCK - 1 - 128, None, "opls"), (128, BLOCK - 128, None, "cos"), (128, BLOCK + 1 - 128, None, "opls"),
               (40, 23, BLOCK - 1, "cos"), (40, 23, BLOCK + 1, "opls"),
               (43692, 21845, None, "opls")]
assert sum(EDGE_SHAPES[-1][:2]) == BLOCK * FINISH + 1


def edge_case(shape, **kw):
    nd, ni, natoms, pair = shape
    return edges(nd, ni, natoms, pair=pair, **kw)


def exact(pair="opls"):
    """case 4: coordinates that are multiples of 0.5.  A planar cis term (phi = 0 exactly) and a planar trans term (phi = pi
    exactly), each as a dihedral and as an improper; a quarter turn (phi = pi / 2); a term whose first three members are collinear
    (A = 0) and one whose members 2 and 3 coincide (g = 0): both contribute exactly nothing"""
    o = np.array([10.0, 20.0, 5.0])
    x = np.array([
        [-0.5, 1.0, 0.0], [0.0, 0.0, 0.0], [1.5, 0.0, 0.0], [2.0, 1.0, 0.0],        # 0-3: cis
        [2.0, -1.0, 0.0],                                                           # 4: with 0-2 trans
        [2.0, 0.0, 1.0],                                                            # 5: with 0-2 a quarter turn
        [4.0, 3.0, 0.0], [5.0, 3.0, 0.0], [6.5, 3.0, 0.0], [7.0, 4.0, 0.0],         # 6-9: 6, 7, 8 collinear
        [0.0, 6.0, 1.0], [1.0, 6.0, 0.0], [1.0, 6.0, 0.0], [2.0, 6.5, 1.0],         # 10-13: 11 and 12 coincide
        [8.0, 8.0, 8.0]]) + o                                                       # 14: in no term
    dihedrals = [[0, 1, 2, 3, 1], [0, 1, 2, 4, 3], [0, 1, 2, 5, 3], [6, 7, 8, 9, 2], [10, 11, 12, 13, 1]]
    impropers = [[0, 1, 2, 3, 1], [0, 1, 2, 4, 1], [9, 8, 7, 6, 2], [10, 11, 12, 13, 2]]
    return _case(f"exact planar and collinear terms, {pair}", x, len(x), dihedrals, impropers, p=PAIRS[pair])


def difference_case():
    """the molecules with their dihedrals alone (opls): d_ev[0] is then the whole energy, whose difference quotient the device-only
    check of tests/test_gpu_dihedral.py compares with the device's own force"""
    c = molecules("opls", True, "image")
    c.impropers = c.impropers[:0]
    c.tag = "molecules (opls dihedrals only), closest image"
    return c


DIFF_H = 1e-4            # A: the step of the device-only check
DIFF_BOUND = 1e-5        # of the largest force component


def gpu_cases():
    """every input the GPU tests use (tests/test_dihedral_ref_math.py holds the float64 restatement to a tenth of the bound on each)"""
    out = [molecules(p, n, f) for p in ("opls", "cos") for f in ("ghost", "image") for n in (True, False)]
    out.append(hub())
    out += [edge_case(e) for e in EDGE_SHAPES]
    out.append(edge_case((129, 128, None, "cos"), newton=False))
    out += [exact("opls"), exact("cos")]
    return out
