"""numpy restatements of the SHAKE rule of include/conp_hip.h (conp_shake_*; LAMMPS FixShake @ 27May2021 without rRESPA, rmass or
RATTLE), and the inputs of the GPU tests.

The rule is written ONCE (class Rule) over a number type, as tests/integrate_ref.py does:
  - Rule("ld"): np.longdouble values that carry their cancellation-free magnitude (class Mag1 below); sqrt(u) has
    m_u / (2 sqrt(u)), what an error of m_u in u moves it by.  The GPU tests bound |got - value| by TOL * magnitude, entry-wise.
  - Rule("f64"): plain float64 in the written order: bit for bit what the kernel does for flags 1 and 3, which use nothing but
    + - * / and comparisons.
    Products and quotients carry FIRST-ORDER magnitudes here (class Mag1): m_a |b| + |a| m_b, not integrate_ref's m_a m_b.  The rule
    is a long chain of products of differences of coordinates (|x| ~ 40 A, |r| ~ 3 A: m / |value| ~ 15 at the start), and m_a m_b
    multiplies these ratios where the errors only add -- after determinant, cofactors and a feedback loop through quad the bound
    would be 10^40 times the value and check nothing.  First order, the loop is a contraction, and so is its magnitude.  Since
    m >= |value| throughout, m_a |b| also covers the product's own rounding.
The clusters of one flag are handled together as arrays; a cluster that is done keeps its values while the others iterate.
"""
import contextlib
from types import SimpleNamespace

import numpy as np

from integrate_ref import BOLTZ, FTM2V, LD, MVV2E, SENTINELS, TOL, Mag, frac, tol_of  # noqa: F401


class Mag1(Mag):
    """a longdouble value with its first-order magnitude (module docstring); sums and differences as integrate_ref.Mag"""
    __slots__ = ()

    @staticmethod
    def of(x):
        return x if isinstance(x, Mag1) else Mag1(x.v, x.m) if isinstance(x, Mag) else Mag1(x)

    def __add__(self, o):
        o = Mag1.of(o)
        return Mag1(self.v + o.v, self.m + o.m)
    __radd__ = __add__

    def __sub__(self, o):
        o = Mag1.of(o)
        return Mag1(self.v - o.v, self.m + o.m)

    def __rsub__(self, o):
        return Mag1.of(o) - self

    def __neg__(self):
        return Mag1(-self.v, self.m)

    def __mul__(self, o):
        o = Mag1.of(o)
        return Mag1(self.v * o.v, self.m * np.abs(o.v) + np.abs(self.v) * o.m)
    __rmul__ = __mul__

    def __truediv__(self, o):
        o = Mag1.of(o)
        return Mag1(self.v / o.v, self.m / np.abs(o.v) + np.abs(self.v) * o.m / (o.v * o.v))

    def __rtruediv__(self, o):
        return Mag1.of(o) / self

    def __getitem__(self, k):
        return Mag1(self.v[k], self.m[k])


@contextlib.contextmanager
def first_order_integrator():
    """integrate_ref.Rule builds its values through its module's name Mag; while this is open that name is Mag1, so that the
    integrator driven by shake's forces (m / |value| ~ 10^4) carries first-order magnitudes too -- with m_a m_b the chain of an nvt
    group overflows within three steps"""
    import integrate_ref
    keep = integrate_ref.Mag
    integrate_ref.Mag = Mag1
    try:
        yield
    finally:
        integrate_ref.Mag = keep


def _where(mask, a, b):
    if isinstance(a, Mag) or isinstance(b, Mag):
        a, b = Mag1.of(a), Mag1.of(b)
        return Mag1(np.where(mask, a.v, b.v), np.where(mask, a.m, b.m))
    return np.where(mask, a, b)

# launch shapes of conp_shake.hip, restated (tests/test_shake_ref_math.py compares them with csrc/conp_kernels.h)
BLOCK = 64        # threads of a workgroup: one cluster each
FINISH = 256      # threads of the finishing workgroup: from BLOCK * FINISH + 1 clusters on a thread adds a second row of partial sums
BIG = BLOCK * FINISH + 1
SIZES = tuple(sorted({1, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 1000, BIG}))
# the cation of the IL decks: types 1, 2, 3 with type 1 the centre; bond types 1 (1-2) and 2 (1-3); angle type 1 (2-1-3)
MASS = np.array([67.07, 15.04, 57.12])
BOND_D = np.array([2.7076, 3.8213])
THETA0 = np.deg2rad(116.035)
ANGLE_D = np.array([float(np.sqrt(BOND_D[0] * BOND_D[0] + BOND_D[1] * BOND_D[1] - 2.0 * BOND_D[0] * BOND_D[1] * np.cos(THETA0)))])
TOLERANCE, MAX_ITER, DT = 1e-4, 10, 2.0


def _v(q):
    return q.v if isinstance(q, Mag) else q


def _sqrt(q):
    if isinstance(q, Mag):
        r = np.sqrt(q.v)
        with np.errstate(divide="ignore", invalid="ignore"):
            return Mag1(r, np.where(q.v > 0, q.m / (2 * np.where(q.v > 0, r, 1)), np.sqrt(q.m)))
    return np.sqrt(q)


def _dot(a, b):
    return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]


def _rows(a, idx):
    """rows idx of an [n][3] array as three columns"""
    r = a[idx]
    return [r[:, 0], r[:, 1], r[:, 2]]


def _put(dst, idx, cols, mask):
    """dst[idx[mask]] = the columns' rows under mask (dst: a float array, or a Mag whose v and m are written)"""
    for c, col in enumerate(cols):
        if isinstance(dst, Mag):
            dst.v[idx[mask], c] = col.v[mask]
            dst.m[idx[mask], c] = col.m[mask]
        else:
            dst[idx[mask], c] = col[mask]


class Rule:
    def __init__(self, kind, c):
        self.ld = kind == "ld"
        self.num = (lambda x: Mag1(x)) if self.ld else (lambda x: np.asarray(x, dtype=np.float64)[()])
        self.c = c
        self.cl = np.asarray(c.cluster, dtype=np.int64).reshape(-1, 7)
        self.m_atom = np.asarray(c.mass, dtype=np.float64)[np.asarray(c.type) - 1]
        self.trace = []      # per solve and flag: (flag, [per iteration (active mask, [|l_new - l| per unknown])]) for the input condition

    def lift(self, a):
        return Mag1.of(a) if self.ld else a

    def copy(self, a):
        return Mag1(a.v.copy(), a.m.copy()) if isinstance(a, Mag) else np.array(a, dtype=np.float64)

    def dtfsq(self, half):
        n, c = self.num, self.c
        return n(0.5) * n(c.dt) * n(c.dt) * n(c.ftm2v) if half else n(c.dt) * n(c.dt) * n(c.ftm2v)

    def diff(self, a, b):
        """a - b per column with one pass of the minimum image"""
        out = []
        for k in range(3):
            d = a[k] - b[k]
            p = float(self.c.prd[k])
            if p > 0:
                big = np.abs(_v(d)) > 0.5 * p
                neg = _v(d) < 0
                d = _where(big & neg, d + self.num(p), _where(big, d - self.num(p), d))
            out.append(d)
        return out

    def _atom(self, i, x, v, f, dtfsq, correct):
        m = self.num(self.m_atom[i])
        im, dtfmsq = self.num(1.0) / m, dtfsq / m
        xi = _rows(x, i)
        if correct:
            zero = self.num(np.zeros(len(i)))
            return SimpleNamespace(i=i, im=im, dtfmsq=dtfmsq, x=xi, xs=xi, f=[zero, zero, zero])
        vi, fi = _rows(v, i), _rows(f, i)
        dtv = self.num(self.c.dt)
        xs = [xi[k] + dtv * vi[k] + dtfmsq * fi[k] for k in range(3)]
        return SimpleNamespace(i=i, im=im, dtfmsq=dtfmsq, x=xi, xs=xs, f=fi)

    def _iterate(self, flag, ainv, quads, dsq, ssq, n):
        """the loop of flags 3 and 1 over K unknowns -> (l [K], done, niter)"""
        K = len(dsq)
        tol = self.c.tolerance
        l = [self.num(np.zeros(n)) for _ in range(K)]
        done = np.zeros(n, dtype=bool)
        niter = np.zeros(n, dtype=np.int64)
        steps = []
        pairs = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)] if K == 3 else [(0, 0), (1, 1), (0, 1)]
        for _ in range(self.c.max_iter):
            active = ~done
            if not active.any():
                break
            b = []
            for k in range(K):
                quad = None
                for q, (i, j) in zip(quads[k], pairs):
                    t = q * l[i] * l[j]
                    quad = t if quad is None else quad + t
                b.append(dsq[k] - ssq[k] - quad)
            new = []
            for k in range(K):
                s = ainv[k][0] * b[0]
                for j in range(1, K):
                    s = s + ainv[k][j] * b[j]
                new.append(s)
            dl = [np.abs(_v(new[k] - l[k])) for k in range(K)]
            now = np.ones(n, dtype=bool)
            for k in range(K):
                now &= ~(dl[k] > tol)
            l = [_where(active, new[k], l[k]) for k in range(K)]
            for k in range(K):
                now |= np.abs(_v(l[k])) > 1e150
            done = np.where(active, now, done)
            niter += active
            steps.append((active.copy(), dl))
        self.trace.append((flag, steps))
        return l, done, niter

    def solve(self, x, v, f, half=False, correct=False):
        """-> SimpleNamespace(f or x as the entry leaves it, vatom [nlocal][6], virial [6], unconverged, bad_determ, niter_max, and per
        flag the multipliers, niter and the clusters' rows).  setup: half=True; correct: half=True, correct=True (v, f ignored)"""
        x = self.lift(x)
        if not correct:
            v, f = self.lift(v), self.lift(f)
        half = half or correct
        dtfsq = self.dtfsq(half)
        n_at = len(self.m_atom)
        out = self.copy(x if correct else f)
        vatom = self.num(np.zeros((n_at, 6)))
        vir = [self.num(0.0) for _ in range(6)]
        res = SimpleNamespace(unconverged=0, bad_determ=0, niter_max=0, flags={})
        ab = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]
        with np.errstate(all="ignore"):
            for flag in (2, 3, 1):
                rows = np.nonzero(self.cl[:, 0] == flag)[0]
                if not len(rows):
                    continue
                cl = self.cl[rows]
                n = len(rows)
                d0 = self.num(self.c.bond_d[cl[:, 4] - 1])
                p0, p1 = (self._atom(cl[:, 1 + k], x, v, f, dtfsq, correct) for k in range(2))
                r01, s01 = self.diff(p0.x, p1.x), self.diff(p0.xs, p1.xs)
                r01sq, s01sq = _dot(r01, r01), _dot(s01, s01)
                im0, im1 = p0.im, p1.im
                if flag == 2:
                    a = (im0 + im1) * (im0 + im1) * r01sq
                    b = 2.0 * (im0 + im1) * _dot(s01, r01)
                    cc = s01sq - d0 * d0
                    determ = b * b - 4.0 * a * cc
                    bad = _v(determ) < 0
                    determ = _where(bad, self.num(np.zeros(n)), determ)
                    root = _sqrt(determ)
                    lam = _where(_v(b) > 0, (-b + root) / (2.0 * a), (-b - root) / (2.0 * a))
                    lam = lam / dtfsq
                    every = np.ones(n, dtype=bool)
                    f0 = [p0.f[k] + lam * r01[k] for k in range(3)]
                    f1 = [p1.f[k] - lam * r01[k] for k in range(3)]
                    vv = [lam * r01[i] * r01[j] for i, j in ab]
                    atoms, forces, solved, nat = [p0, p1], [f0, f1], every, 2.0
                    res.bad_determ += int(bad.sum())
                    res.flags[2] = SimpleNamespace(rows=rows, lam=[lam], niter=np.zeros(n, dtype=np.int64), bad=bad, unconverged=~every)
                else:
                    p2 = self._atom(cl[:, 3], x, v, f, dtfsq, correct)
                    im2 = p2.im
                    d1 = self.num(self.c.bond_d[cl[:, 5] - 1])
                    r02, s02 = self.diff(p0.x, p2.x), self.diff(p0.xs, p2.xs)
                    r02sq, s02sq = _dot(r02, r02), _dot(s02, s02)
                    r0102 = _dot(r01, r02)
                    if flag == 3:
                        a11 = 2.0 * (im0 + im1) * _dot(s01, r01)
                        a12 = 2.0 * im0 * _dot(s01, r02)
                        a21 = 2.0 * im0 * _dot(s02, r01)
                        a22 = 2.0 * (im0 + im2) * _dot(s02, r02)
                        determ = a11 * a22 - a12 * a21
                        solved = _v(determ) != 0
                        determinv = self.num(1.0) / _where(solved, determ, self.num(np.ones(n)))
                        ainv = [[a22 * determinv, -a12 * determinv], [-a21 * determinv, a11 * determinv]]
                        quads = [[(im0 + im1) * (im0 + im1) * r01sq, im0 * im0 * r02sq, 2.0 * (im0 + im1) * im0 * r0102],
                                 [im0 * im0 * r01sq, (im0 + im2) * (im0 + im2) * r02sq, 2.0 * (im0 + im2) * im0 * r0102]]
                        l, done, niter = self._iterate(3, ainv, quads, [d0 * d0, d1 * d1], [s01sq, s02sq], n)
                        raw, l = l, [q / dtfsq for q in l]
                        f0 = [p0.f[k] + (l[0] * r01[k] + l[1] * r02[k]) for k in range(3)]
                        f1 = [p1.f[k] - l[0] * r01[k] for k in range(3)]
                        f2 = [p2.f[k] - l[1] * r02[k] for k in range(3)]
                        vv = [l[0] * r01[i] * r01[j] + l[1] * r02[i] * r02[j] for i, j in ab]
                    else:
                        d2 = self.num(self.c.angle_d[cl[:, 6] - 1])
                        r12, s12 = self.diff(p1.x, p2.x), self.diff(p1.xs, p2.xs)
                        r12sq, s12sq = _dot(r12, r12), _dot(s12, s12)
                        r0112, r0212 = _dot(r01, r12), _dot(r02, r12)
                        a11 = 2.0 * (im0 + im1) * _dot(s01, r01)
                        a12 = 2.0 * im0 * _dot(s01, r02)
                        a13 = -2.0 * im1 * _dot(s01, r12)
                        a21 = 2.0 * im0 * _dot(s02, r01)
                        a22 = 2.0 * (im0 + im2) * _dot(s02, r02)
                        a23 = 2.0 * im2 * _dot(s02, r12)
                        a31 = -2.0 * im1 * _dot(s12, r01)
                        a32 = 2.0 * im2 * _dot(s12, r02)
                        a33 = 2.0 * (im1 + im2) * _dot(s12, r12)
                        determ = a11 * a22 * a33 + a12 * a23 * a31 + a13 * a21 * a32 - a11 * a23 * a32 - a12 * a21 * a33 - a13 * a22 * a31
                        solved = _v(determ) != 0
                        determinv = self.num(1.0) / _where(solved, determ, self.num(np.ones(n)))
                        ainv = [[determinv * (a22 * a33 - a23 * a32), -determinv * (a12 * a33 - a13 * a32), determinv * (a12 * a23 - a13 * a22)],
                                [-determinv * (a21 * a33 - a23 * a31), determinv * (a11 * a33 - a13 * a31), -determinv * (a11 * a23 - a13 * a21)],
                                [determinv * (a21 * a32 - a22 * a31), -determinv * (a11 * a32 - a12 * a31), determinv * (a11 * a22 - a12 * a21)]]
                        quads = [[(im0 + im1) * (im0 + im1) * r01sq, im0 * im0 * r02sq, im1 * im1 * r12sq,
                                  2.0 * (im0 + im1) * im0 * r0102, -2.0 * (im0 + im1) * im1 * r0112, -2.0 * im0 * im1 * r0212],
                                 [im0 * im0 * r01sq, (im0 + im2) * (im0 + im2) * r02sq, im2 * im2 * r12sq,
                                  2.0 * (im0 + im2) * im0 * r0102, 2.0 * im0 * im2 * r0112, 2.0 * (im0 + im2) * im2 * r0212],
                                 [im1 * im1 * r01sq, im2 * im2 * r02sq, (im1 + im2) * (im1 + im2) * r12sq,
                                  -2.0 * im1 * im2 * r0102, -2.0 * (im1 + im2) * im1 * r0112, 2.0 * (im1 + im2) * im2 * r0212]]
                        l, done, niter = self._iterate(1, ainv, quads, [d0 * d0, d1 * d1, d2 * d2], [s01sq, s02sq, s12sq], n)
                        raw, l = l, [q / dtfsq for q in l]
                        f0 = [p0.f[k] + (l[0] * r01[k] + l[1] * r02[k]) for k in range(3)]
                        f1 = [p1.f[k] - (l[0] * r01[k] - l[2] * r12[k]) for k in range(3)]
                        f2 = [p2.f[k] - (l[1] * r02[k] + l[2] * r12[k]) for k in range(3)]
                        vv = [l[0] * r01[i] * r01[j] + l[1] * r02[i] * r02[j] + l[2] * r12[i] * r12[j] for i, j in ab]
                    zero = self.num(np.zeros(n))
                    vv = [_where(solved, q, zero) for q in vv]
                    niter = np.where(solved, niter, 0)
                    unconv = solved & ~done
                    atoms, forces, nat = [p0, p1, p2], [f0, f1, f2], 3.0
                    res.bad_determ += int((~solved).sum())
                    res.unconverged += int(unconv.sum())
                    res.niter_max = max(res.niter_max, int(niter.max()))
                    # eq: what the multipliers solve, before the division by dtfsq:  sum_j a[k][j] l_j + quad_k(l) = d_k^2 - s_k^2
                    res.flags[flag] = SimpleNamespace(
                        rows=rows, lam=l, raw=raw, niter=niter, bad=~solved, unconverged=unconv, quads=quads,
                        dsq=[d0 * d0, d1 * d1] + ([d2 * d2] if flag == 1 else []), ssq=[s01sq, s02sq] + ([s12sq] if flag == 1 else []),
                        a=[[a11, a12], [a21, a22]] if flag == 3 else [[a11, a12, a13], [a21, a22, a23], [a31, a32, a33]])
                for p, fo in zip(atoms, forces):
                    if correct:
                        fo = [p.x[k] + p.dtfmsq * fo[k] for k in range(3)]
                    _put(out, p.i, fo, solved)
                    _put6(vatom, p.i, [q / nat for q in vv])
                for k in range(6):
                    vir[k] = vir[k] + (Mag1(vv[k].v.sum(), vv[k].m.sum()) if self.ld else np.float64(vv[k].sum()))
        res.out, res.vatom, res.virial = out, vatom, vir
        return res

    def d_out(self, res):
        """the nine d_out entries -> (values, magnitudes) (f64: magnitudes None)"""
        tail = [res.unconverged, res.bad_determ, res.niter_max]
        if self.ld:
            return (np.array([q.v for q in res.virial] + tail, dtype=LD), np.array([q.m for q in res.virial] + [0, 0, 0], dtype=LD))
        return np.array([float(q) for q in res.virial] + tail, dtype=np.float64), None

    def check(self, x):
        """-> (largest |r - d| / d over the bonds, over the 1-2 distances of the flag-1 clusters), longdouble"""
        x = np.asarray(x.v if isinstance(x, Mag) else x, dtype=LD)
        keep = self.ld
        self.ld, num = False, self.num
        self.num = lambda q: np.asarray(q, dtype=LD)
        bond, angle = LD(0), LD(0)
        for flag in (2, 3, 1):
            cl = self.cl[self.cl[:, 0] == flag]
            if not len(cl):
                continue
            x0, x1 = _rows(x, cl[:, 1]), _rows(x, cl[:, 2])
            r = self.diff(x0, x1)
            d = self.c.bond_d[cl[:, 4] - 1].astype(LD)
            bond = max(bond, (np.abs(np.sqrt(_dot(r, r)) - d) / d).max())
            if flag != 2:
                x2 = _rows(x, cl[:, 3])
                r = self.diff(x0, x2)
                d = self.c.bond_d[cl[:, 5] - 1].astype(LD)
                bond = max(bond, (np.abs(np.sqrt(_dot(r, r)) - d) / d).max())
                if flag == 1:
                    r = self.diff(x1, x2)
                    d = self.c.angle_d[cl[:, 6] - 1].astype(LD)
                    angle = max(angle, (np.abs(np.sqrt(_dot(r, r)) - d) / d).max())
        self.ld, self.num = keep, num
        return bond, angle


def _put6(dst, idx, cols):
    for c, col in enumerate(cols):
        if isinstance(dst, Mag):
            dst.v[idx, c] = col.v
            dst.m[idx, c] = col.m
        else:
            dst[idx, c] = col


def clear_of_the_tolerance(R, tolerance):
    """the input condition of the GPU tests: at every iteration of every cluster of the solves R (a Rule("ld")) has made, each
    |l_new - l| is further than 1e-9 tolerance from the tolerance -> the smallest distance found, in units of the tolerance"""
    near = np.inf
    for _flag, steps in R.trace:
        for active, dl in steps:
            for d in dl:
                if active.any():
                    near = min(near, float(np.abs(d[active] - tolerance).min()) / tolerance)
    return near


# ---- input builders -----------------------------------------------------------------------------------------------------------------
def case(tag, ncluster, flags, seed=0, prd=(0.0, 0.0, 0.0), noise=0.05, max_iter=MAX_ITER, box=40.0, centres=None, wrap=False, free=0.1):
    """ncluster clusters with flags drawn from `flags`, the cation's ideal geometry in a random orientation with every coordinate
    moved by up to `noise` A (a few percent of the distances); a fraction `free` of the atoms (at least one) in no cluster; atom
    indices permuted, so that the members of a cluster lie anywhere; SENTINELS rows behind nlocal in x, v, f.  Real units,
    velocities thermal at 400 K, forces of the size of a deck's.  Unused fields of a cluster record hold junk (-7, 99)"""
    rng = np.random.default_rng(7000 + seed)
    flag = rng.choice(np.asarray(flags), size=ncluster) if ncluster else np.zeros(0, dtype=np.int64)
    nat = np.where(flag == 2, 2, 3)
    nin = int(nat.sum())
    nfree = max(1, int(np.ceil(free * nin / (1.0 - free))))
    nlocal = nin + nfree
    slot = rng.permutation(nlocal)
    first = np.concatenate([[0], np.cumsum(nat)])[:-1] if ncluster else np.zeros(0, dtype=np.int64)
    cluster = np.full((ncluster, 7), 99, dtype=np.int32)
    cluster[:, 3] = -7
    typ = rng.integers(1, 4, nlocal).astype(np.int32)
    x = rng.uniform(0.0, box, (nlocal + SENTINELS, 3))
    x0 = rng.uniform(0.0, box, (ncluster, 3)) if centres is None else np.asarray(centres, dtype=np.float64)
    u = rng.normal(size=(ncluster, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    w = np.cross(u, rng.normal(size=(ncluster, 3))); w /= np.linalg.norm(w, axis=1)[:, None]
    pos = [x0, x0 + BOND_D[0] * u, x0 + BOND_D[1] * (np.cos(THETA0) * u + np.sin(THETA0) * w)]
    for k in range(ncluster):
        i = slot[first[k]:first[k] + nat[k]]
        cluster[k, 0] = flag[k]
        cluster[k, 1:1 + nat[k]] = i
        cluster[k, 4] = 1
        if flag[k] != 2:
            cluster[k, 5] = 2
        if flag[k] == 1:
            cluster[k, 6] = 1
        for m in range(nat[k]):
            typ[i[m]] = m + 1
            x[i[m]] = pos[m][k] + rng.uniform(-noise, noise, 3)
    if wrap:
        for c in range(3):
            if prd[c] > 0:
                x[:nlocal, c] -= prd[c] * np.floor(x[:nlocal, c] / prd[c])
    m_all = np.concatenate([MASS[typ - 1], np.full(SENTINELS, MASS[0])])
    v = rng.normal(size=(nlocal + SENTINELS, 3)) * np.sqrt(BOLTZ * 400.0 / (m_all * MVV2E))[:, None]
    f = rng.normal(size=(nlocal + SENTINELS, 3)) * 10.0
    member = np.zeros(nlocal, dtype=bool)
    for k in range(ncluster):
        member[cluster[k, 1:1 + nat[k]]] = True
    return SimpleNamespace(tag=tag, nlocal=int(nlocal), ncluster=int(ncluster), type=typ, mass=MASS.copy(), bond_d=BOND_D.copy(),
                           angle_d=ANGLE_D.copy(), cluster=cluster, tolerance=TOLERANCE, max_iter=int(max_iter), dt=DT, ftm2v=FTM2V,
                           prd=np.asarray(prd, dtype=np.float64), x=np.ascontiguousarray(x), v=np.ascontiguousarray(v),
                           f=np.ascontiguousarray(f), member=member, seed=seed)


def ladder_case(flag, n):
    return case(f"flag {flag}, {n} clusters", n, [flag], seed=10 * (n % 1000) + flag)


def mixed_case():
    return case("flags 1, 2 and 3 interleaved, 300 clusters", 300, [1, 2, 3], seed=5)


def straddle_case(where):
    """16 flag-1 clusters with their centres within 1 A of the faces named in `where` ('x', 'y', 'z' or 'xyz': a corner) of a 40 A
    box, coordinates wrapped into the box, so that their members lie on both sides"""
    rng = np.random.default_rng(90 + len(where) + ord(where[0]))
    cen = rng.uniform(5.0, 35.0, (16, 3))
    for ch in where:
        cen[:, "xyz".index(ch)] = rng.uniform(-1.0, 1.0, 16)
    return case(f"straddling {where}", 16, [1], seed=20 + ord(where[0]) + len(where), prd=(40.0, 40.0, 40.0), centres=cen, wrap=True)


def unwrapped(c):
    """the same input with every cluster's members moved next to its first atom and prd = 0"""
    d = SimpleNamespace(**vars(c))
    d.x = c.x.copy()
    for row in c.cluster:
        for m in (2, 3):
            if row[0] == 2 and m == 3:
                continue
            for k in range(3):
                if c.prd[k] > 0:
                    d.x[row[m], k] -= c.prd[k] * np.round((d.x[row[m], k] - d.x[row[1], k]) / c.prd[k])
    d.prd = np.zeros(3)
    d.tag = c.tag + ", unwrapped"
    return d


def with_(c, **k):
    d = SimpleNamespace(**vars(c))
    for key, val in k.items():
        setattr(d, key, val)
    return d


def gpu_cases():
    """every input of tests/test_gpu_shake.py whose iteration count the bit-for-bit comparison depends on"""
    out = [ladder_case(flag, n) for flag in (1, 3, 2) for n in SIZES]
    out.append(mixed_case())
    out += [straddle_case(w) for w in ("x", "y", "z", "xyz")]
    return out


def strong_case(max_iter):
    """8 clusters of flags 1 and 3 with every coordinate moved by up to 0.4 A: nothing converges in one or two iterations"""
    return case(f"strongly distorted, max_iter {max_iter}", 8, [1, 3], seed=31, noise=0.4, max_iter=max_iter)


def special_case():
    """six ordinary clusters, then three constructed ones (prd = 0, f = 0 on their atoms):
      - flag 3 and flag 1 with s01 perpendicular to r01, r02 and r12: the first row of the matrix is 0 and determ == 0 exactly;
      - flag 2 with s01 perpendicular to r01 and |s01| = 5 A > d0: b = 0, c > 0, so the discriminant -4 a c is negative.
    x1 - x0 = (e, 0, 0) and x2 - x0 = (0, e', 0) are exact differences, and v0 = (e / 2, 0, z / 2) with dt = 2 makes
    xs0 - xs1 = (0, 0, z) exactly"""
    b = case("ordinary", 6, [1, 3, 2], seed=41)
    n0 = b.nlocal
    new_x, new_v, new_t, rows = [], [], [], []
    for flag, px, z in ((3, 8.0, 0.6), (1, 14.0, 0.6), (2, 20.0, 5.0)):
        p = np.array([px, 8.0, 8.0])
        x1 = p + np.array([BOND_D[0], 0.0, 0.0])
        x2 = p + np.array([0.0, BOND_D[1], 0.0])
        e = x1[0] - p[0]
        i = n0 + len(new_x)
        new_x += [p, x1] + ([x2] if flag != 2 else [])
        new_v += [np.array([e / 2.0, 0.0, z / 2.0]), np.zeros(3)] + ([np.zeros(3)] if flag != 2 else [])
        new_t += [1, 2] + ([3] if flag != 2 else [])
        rows.append([flag, i, i + 1, i + 2 if flag != 2 else -7, 1, 2 if flag != 2 else 99, 1 if flag == 1 else 99])
    k = len(new_x)
    ins = lambda a, new: np.ascontiguousarray(np.concatenate([a[:n0], np.array(new, dtype=a.dtype).reshape((k,) + a.shape[1:]), a[n0:]]))
    return with_(b, tag="constructed determinants", nlocal=n0 + k, ncluster=b.ncluster + 3, x=ins(b.x, new_x), v=ins(b.v, new_v),
                 f=ins(b.f, np.zeros((k, 3))), type=ins(b.type, new_t), cluster=np.concatenate([b.cluster, np.array(rows, dtype=np.int32)]),
                 member=np.concatenate([b.member, np.ones(k, dtype=bool)]), first_special=b.ncluster)


def deck_case():
    """the 320 cations of tests/golden/deck_il.npz as flag-1 clusters: the members of a molecule are its atoms of types 1 (the centre),
    2 and 3; the file's coordinates are wrapped in x and y, so molecules lie across the box.  All 3776 atoms are owned; anions and
    electrodes are in no cluster"""
    import os
    d = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "deck_il.npz"))
    typ, mol = d["type"].astype(np.int32), d["mol"]
    n = len(typ)
    rows = []
    for m in np.unique(mol[typ == 1]):
        at = np.nonzero(mol == m)[0]
        i0, i1, i2 = (at[typ[at] == t] for t in (1, 2, 3))
        assert len(i0) == len(i1) == len(i2) == 1
        rows.append([1, i0[0], i1[0], i2[0], 1, 2, 1])
    prd = d["boxhi"] - d["boxlo"]
    prd[2] = 0.0
    rng = np.random.default_rng(320)
    mass = np.array([67.07, 15.04, 57.12, 144.96, 12.001])
    x = np.concatenate([d["x"], rng.uniform(0.0, 30.0, (SENTINELS, 3))])
    m_all = np.concatenate([mass[typ - 1], np.full(SENTINELS, mass[0])])
    v = rng.normal(size=(n + SENTINELS, 3)) * np.sqrt(BOLTZ * 400.0 / (m_all * MVV2E))[:, None]
    f = rng.normal(size=(n + SENTINELS, 3)) * 10.0
    cluster = np.array(rows, dtype=np.int32)
    member = np.zeros(n, dtype=bool)
    member[cluster[:, 1:4].ravel()] = True
    return SimpleNamespace(tag="the cations of the IL deck", nlocal=n, ncluster=len(rows), type=typ, mass=mass, bond_d=BOND_D.copy(),
                           angle_d=ANGLE_D.copy(), cluster=cluster, tolerance=TOLERANCE, max_iter=MAX_ITER, dt=DT, ftm2v=FTM2V, prd=prd,
                           x=np.ascontiguousarray(x), v=np.ascontiguousarray(v), f=np.ascontiguousarray(f), member=member, seed=320)


def step_case(style):
    """150 clusters of all three flags wrapped into a periodic 40 A box, a harmonic angle over every flag-3 cluster (its two bonds are
    constrained, its angle is not: the cond2 deck), every atom in one group of the given style (0 nve, 1 nvt)"""
    c = case(f"device steps, {'nvt' if style else 'nve'}", 150, [1, 3, 2], seed=61 + style, prd=(40.0, 40.0, 40.0), wrap=True)
    three = c.cluster[c.cluster[:, 0] == 3]
    c.angles = np.stack([three[:, 2], three[:, 1], three[:, 3], np.ones(len(three), dtype=np.int32)], axis=1).astype(np.int32)
    c.p = SimpleNamespace(bond_k=np.array([450.0]), bond_r0=np.array([1.0]), angle_k=np.array([55.0]), angle_theta0=np.array([THETA0]))
    nconstraint = int(np.where(c.cluster[:, 0] == 2, 1, np.where(c.cluster[:, 0] == 3, 2, 3)).sum())
    c.integ = SimpleNamespace(type=c.type, group=np.zeros(c.nlocal, dtype=np.int32), mass=c.mass, style=np.array([style], dtype=np.int32),
                              dof=np.array([3.0 * c.nlocal - 3.0 - nconstraint]), t_period=np.array([100.0]), dt=c.dt, ftm2v=c.ftm2v,
                              mvv2e=MVV2E, boltz=BOLTZ, t_target=np.array([400.0]))
    return c


def reference_steps(c, steps=3):
    """the longdouble run of: correct -> bonded -> shake setup -> integrate setup -> steps x (initial -> [check] -> bonded -> shake
    post_force -> final), the bonded forces from tests/bonded_ref.py at the reference's x rounded to float64
    -> SimpleNamespace(x, v, f (Mag), check [steps] (bond, 1-2), d_out rows of the last final, shake (value, magnitude) of the last
    post_force, near: the input condition over every solve of the run)"""
    import bonded_ref as br
    import integrate_ref as ir
    n = c.nlocal
    with first_order_integrator():
        S, I = Rule("ld", c), ir.Rule("ld", c.integ)

    def bonded(x):
        fr = br.reference(x.v.astype(np.float64), n, None, c.angles, c.p, True, c.prd)
        return Mag1(fr.f, fr.A)
    with first_order_integrator():
        x = S.solve(c.x[:n], None, None, correct=True).out
        f = S.solve(x, c.v[:n], bonded(x), half=True).out
        I.setup(c.v[:n], c.integ.t_target)
        v, dev = c.v[:n], []
        for _ in range(steps):
            x, v = I.initial(x, v, f, c.integ.t_target)
            dev.append(S.check(x))
            res = S.solve(x, v, bonded(x))
            f = res.out
            v, rows = I.final(v, f)
    return SimpleNamespace(x=x, v=v, f=f, check=dev, rows=rows, shake=S.d_out(res), near=clear_of_the_tolerance(S, c.tolerance))
