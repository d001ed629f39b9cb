"""numpy reference (np.longdouble) of the lj/cut/coul/long pair loop over a LAMMPS half list, straight from the definitions in
include/conp_hip.h (conp_pair_compute; LAMMPS pair_lj_cut_coul_long.cpp @ 27May2021 without tables, Pair::ev_tally).

reference(...) returns the results (f, eng, W, eatom, vatom) and the cancellation-free magnitudes the bounds of the GPU tests are
stated against: A[nall] (forces), E_abs, W_abs[6], eatom_abs[nall], vatom_abs[nall][6] -- the same sums with the absolute value of
every term.  The 5-term erfc polynomial is part of the definition (as for the A matrix, tests/helpers.py)."""
from types import SimpleNamespace

import numpy as np

LD = np.longdouble
NEIGHMASK = 0x3FFFFFFF
SPECIAL_COUL = (1.0, 0.0, 0.5, 0.8333)
SPECIAL_LJ = (1.0, 0.0, 0.0, 0.5)
ONES = (1.0, 1.0, 1.0, 1.0)
SEED = 4          # systems.small_random(ne_side=4, n_elyte=64, seed=SEED): the smallest listed distance is 0.815 A (seeds 1-12 scanned)
_P, _A = LD("0.3275911"), [LD(s) for s in ("0.254829592", "-0.284496736", "1.421413741", "-1.453152027", "1.061405429")]
# the library's constants are doubles: the decimal strings above rounded to double
_P, _A = LD(float(_P)), [LD(float(a)) for a in _A]
_F = LD(1.12837917)


def erfc_poly(x, e):
    t = 1 / (1 + _P * x)
    return t * (_A[0] + t * (_A[1] + t * (_A[2] + t * (_A[3] + t * _A[4])))) * e


def lj_tables(ntypes, cutoff, seed=3, with_lj=True):
    """deterministic synthetic pair_coeff tables [(ntypes+1), (ntypes+1)]: epsilon in 0.05-0.4, sigma in 2.5-3.5 per type, arithmetic
    mixing, cut_lj per type pair 0.6 / 0.8 / 1.0 of the cutoff (so the LJ and the Coulomb gate differ), energy shifted (offset != 0);
    cutsq = max(cut_lj, cut_coul)^2 = cutoff^2"""
    n = ntypes + 1
    p = SimpleNamespace(ntypes=ntypes, cut_coul=float(cutoff), cutsq=np.full((n, n), float(cutoff) ** 2), lj=None)
    if not with_lj:
        return p
    rng = np.random.default_rng(seed)
    eps, sig = rng.uniform(0.05, 0.4, n), rng.uniform(2.5, 3.5, n)
    e = np.sqrt(eps[:, None] * eps[None, :])
    s = 0.5 * (sig[:, None] + sig[None, :])
    pick = rng.integers(0, 3, (n, n))
    pick = np.triu(pick) + np.triu(pick, 1).T
    cut = np.array([0.6, 0.8, 1.0])[pick] * cutoff
    p.lj = dict(cut_ljsq=cut * cut, lj1=48 * e * s ** 12, lj2=24 * e * s ** 6, lj3=4 * e * s ** 12, lj4=4 * e * s ** 6,
                offset=4 * e * ((s / cut) ** 12 - (s / cut) ** 6))
    assert np.all(p.lj["offset"] != 0)
    return p


def pairs_of(lst):
    """(i, jraw) of every listed pair, row by row"""
    own = np.asarray(lst.ilist[:lst.inum], dtype=np.int64)
    cnt = lst.numneigh[own].astype(np.int64)
    i = np.repeat(own, cnt)
    start = np.repeat(lst.first[own].astype(np.int64), cnt)
    within = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return i, lst.neigh[start + within].astype(np.int64) & 0xFFFFFFFF


def reference(x, q, typ, nlocal, lst, p, g_ewald, qqrd2e, newton, special_lj=ONES, special_coul=ONES):
    x, q = np.asarray(x, dtype=LD), np.asarray(q, dtype=LD)
    nall = len(q)
    g, qs = LD(g_ewald), LD(qqrd2e)
    i, jraw = pairs_of(lst)
    sb, j = (jraw >> 30) & 3, jraw & NEIGHMASK
    fc, fl = np.asarray(special_coul, dtype=LD)[sb], np.asarray(special_lj, dtype=LD)[sb]
    d = x[i] - x[j]
    rsq = (d * d).sum(axis=1)
    ti, tj = typ[i], typ[j]
    keep = rsq < p.cutsq[ti, tj].astype(LD)
    i, j, fc, fl, d, rsq, ti, tj = i[keep], j[keep], fc[keep], fl[keep], d[keep], rsq[keep], ti[keep], tj[keep]
    r2inv = 1 / rsq
    r = np.sqrt(rsq)
    # Coulomb
    cin = rsq < LD(p.cut_coul) * LD(p.cut_coul)
    xx = g * r
    e = np.exp(-xx * xx)
    pre = np.where(cin, qs * q[i] * q[j] / r, LD(0))
    erfc = erfc_poly(xx, e)
    sub = np.where(fc < 1, (1 - fc) * pre, LD(0))
    forcecoul = pre * (erfc + _F * xx * e) - sub
    ecoul = pre * erfc - sub
    mag_fc = np.abs(pre) * (erfc + _F * xx * e) + np.abs(sub)
    mag_ec = np.abs(pre) * erfc + np.abs(sub)
    # LJ
    z = np.zeros(len(r), dtype=LD)
    forcelj, evdwl, mag_fl, mag_el = z, z, z, z
    if p.lj is not None:
        T = {k: v[ti, tj].astype(LD) for k, v in p.lj.items()}
        lin = rsq < T["cut_ljsq"]
        r6 = r2inv ** 3
        forcelj = np.where(lin, r6 * (T["lj1"] * r6 - T["lj2"]), LD(0))
        evdwl = np.where(lin, fl * (r6 * (T["lj3"] * r6 - T["lj4"]) - T["offset"]), LD(0))
        mag_fl = np.where(lin, fl * r6 * (T["lj1"] * r6 + T["lj2"]), LD(0))
        mag_el = np.where(lin, fl * (r6 * (T["lj3"] * r6 + T["lj4"]) + np.abs(T["offset"])), LD(0))
    fpair = (forcecoul + fl * forcelj) * r2inv
    mag_fp = (mag_fc + mag_fl) * r2inv
    iw = np.full(len(i), True) if newton else i < nlocal
    jw = np.full(len(j), True) if newton else j < nlocal
    w = np.ones(len(i), dtype=LD) if newton else (LD(0.5) * (i < nlocal) + LD(0.5) * (j < nlocal))
    prod = np.stack([d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2], d[:, 0] * d[:, 1], d[:, 0] * d[:, 2], d[:, 1] * d[:, 2]], 1)

    def scatter(shape, vi, vj):
        out = np.zeros(shape, dtype=LD)
        np.add.at(out, i[iw], vi[iw])
        np.add.at(out, j[jw], vj[jw])
        return out
    f = scatter((nall, 3), d * fpair[:, None], -d * fpair[:, None])
    A = scatter((nall,), r * mag_fp, r * mag_fp)
    eh, ehm = (evdwl + ecoul) / 2, (mag_el + mag_ec) / 2
    eatom, eatom_abs = scatter((nall,), eh, eh), scatter((nall,), ehm, ehm)
    vh, vhm = prod * (fpair / 2)[:, None], np.abs(prod) * (mag_fp / 2)[:, None]
    vatom, vatom_abs = scatter((nall, 6), vh, vh), scatter((nall, 6), vhm, vhm)
    eng = np.array([(w * evdwl).sum(), (w * ecoul).sum()], dtype=LD)
    W = (prod * (w * fpair)[:, None]).sum(axis=0)
    return SimpleNamespace(f=f, eng=eng, W=W, eatom=eatom, vatom=vatom, A=A, E_abs=(w * (mag_el + mag_ec)).sum(),
                           W_abs=(np.abs(prod) * (w * mag_fp)[:, None]).sum(axis=0), eatom_abs=eatom_abs, vatom_abs=vatom_abs,
                           npairs=int(len(i)), rmin=float(r.min()) if len(r) else np.inf, r=r, i=i, j=j,
                           terms=SimpleNamespace(pre=pre, fc=fc, fl=fl, evdwl=evdwl, forcelj=forcelj, w=w, d=d, r2inv=r2inv, iw=iw, jw=jw))


def for_atoms(at, lst, p, s, newton, special_lj=ONES, special_coul=ONES, typ=None, q=None, x=None):
    """reference() on a neighbor.Atoms / NeighList / systems.System triple"""
    from conp_amd import systems
    return reference(at.x if x is None else x, at.q if q is None else q, at.type if typ is None else typ, at.nlocal, lst, p,
                     s.g_ewald, systems.QQRD2E, newton, special_lj, special_coul)


def fold(v, owner, nlocal):
    """ghost entries added onto their owners: what LAMMPS' reverse communication does (one rank, periodic images)"""
    out = np.zeros((nlocal,) + v.shape[1:], dtype=v.dtype)
    np.add.at(out, owner, v)
    return out
