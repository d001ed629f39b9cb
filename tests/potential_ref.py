"""numpy reference (np.longdouble) of the pair part of `compute potential/atom` and of its finishing formula, from the definitions in
include/conp_hip.h (conp_compute_potential_atom, conp_potential_atom_device).

pair_loop(...) restates the reference's loop over a half list (compute_potential_atom.cpp:223-308): every listed pair that passes
the three gates -- one member selected; one member charged; newton, or the owner selected, or the neighbour owned -- adds
q_j dudq to a selected owner and q_i dudq to a neighbour that can receive (owned, or any row with newton on).  Unselected rows
collect partial sums there, as in the reference; only selected rows mean anything.
pair_gather(...) restates the device entry's form: per selected row that can receive, its own row and then its transposed entries
(tests/transpose_ref.py), partners without charge skipped, nothing written on the other rows.
pair_direct(...) is the definition without any list: every selected owned atom against every periodic image of every owned atom.
All three return (pot, A): the sums in e / A (no volts factor) and the cancellation-free magnitudes A_a = sum |q_b dudq| the GPU
tests state their bounds against.  finish(...) is the tail of the compute: k-space part, Gaussian self term, slab terms, volts."""
import itertools

import numpy as np

import transpose_ref as tr
from pair_force_ref import LD, NEIGHMASK, erfc_poly, pairs_of

RSQ_FLOOR = LD(1e-10)             # the double 1e-10 (compute_potential_atom.cpp:255)
ERFC_MAX = LD(5.8)
SQRT2 = np.sqrt(LD(2))
PIS = np.sqrt(LD(np.pi))          # sqrt of the double pi: the library's sqrt(pi) constant to 1e-16


def cut_coulsq_of(cutoff, g_ewald):
    """the reference's min(cut_coul, 5.8 / g)^2 (compute_potential_atom.cpp:246-249), in float64 as the library forms it"""
    return min(float(cutoff) * float(cutoff), 5.8 * 5.8 / (float(g_ewald) * float(g_ewald)))


def dudq_of(rsq, ne2, g_ewald, eta):
    """dudq of pairs at rsq (already floored) with ne2 eta members: erfc(g r) / r, minus erfc(eta' r) / r behind the 5.8 gate"""
    r = np.sqrt(rsq)
    x = LD(g_ewald) * r
    out = erfc_poly(x, np.exp(-x * x)) / r
    if eta != 0.0:
        xe = np.where(ne2 == 2, LD(eta) * r / SQRT2, LD(eta) * r)
        on = (ne2 > 0) & (xe < ERFC_MAX)
        out = out - np.where(on, erfc_poly(xe, np.exp(-xe * xe)) / r, LD(0))
    return out


def _pairs(x, q, typ, flags, lst, cutsq, cut_coulsq, g_ewald, eta):
    """every listed pair inside both cutoffs: (i, j, dudq), special bits masked off"""
    i, jraw = pairs_of(lst)
    j = jraw & NEIGHMASK
    d = x[i] - x[j]
    rsq = np.maximum((d * d).sum(axis=1), RSQ_FLOOR)
    keep = (rsq < np.asarray(cutsq)[typ[i], typ[j]].astype(LD)) & (rsq < LD(cut_coulsq))
    i, j, rsq = i[keep], j[keep], rsq[keep]
    eb = (np.asarray(flags) >> 1) & 1
    return i, j, dudq_of(rsq, eb[i] + eb[j], g_ewald, eta)


def pair_loop(x, q, typ, flags, nlocal, lst, cutsq, cut_coulsq, g_ewald, eta, newton):
    x, q, flags = np.asarray(x, dtype=LD), np.asarray(q, dtype=LD), np.asarray(flags)
    nall = len(q)
    sel = (flags & 1) != 0
    i, j, dudq = _pairs(x, q, typ, flags, lst, cutsq, cut_coulsq, g_ewald, eta)
    gate = (sel[i] | sel[j]) & ((q[i] != 0) | (q[j] != 0)) & (bool(newton) | sel[i] | (j < nlocal))
    i, j, dudq = i[gate], j[gate], dudq[gate]
    pot, A = np.zeros(nall, dtype=LD), np.zeros(nall, dtype=LD)
    mine = sel[i]
    np.add.at(pot, i[mine], (q[j] * dudq)[mine]); np.add.at(A, i[mine], np.abs(q[j] * dudq)[mine])
    recv = (j < nlocal) | bool(newton)
    np.add.at(pot, j[recv], (q[i] * dudq)[recv]); np.add.at(A, j[recv], np.abs(q[i] * dudq)[recv])
    return pot, A


def pair_gather(x, q, typ, flags, nlocal, lst, cutsq, cut_coulsq, g_ewald, eta, newton):
    x, q, flags = np.asarray(x, dtype=LD), np.asarray(q, dtype=LD), np.asarray(flags)
    nall = len(q)
    ntotal = nall if newton else nlocal
    own_row, tr_ptr, tr_entry = tr.transpose(lst, nall)
    eb = (flags >> 1) & 1
    cs = np.asarray(cutsq)
    pot, A = np.zeros(nall, dtype=LD), np.zeros(nall, dtype=LD)

    def terms(owner, other, charge_of):
        """q_charge_of dudq of the pairs (owner[k], other[k]) in the owner's orientation, partners without charge dropped"""
        ok = q[charge_of] != 0
        owner, other, charge_of = owner[ok], other[ok], charge_of[ok]
        d = x[owner] - x[other]
        rsq = np.maximum((d * d).sum(axis=1), RSQ_FLOOR)
        keep = (rsq < cs[typ[owner], typ[other]].astype(LD)) & (rsq < LD(cut_coulsq))
        return q[charge_of[keep]] * dudq_of(rsq[keep], (eb[owner] + eb[other])[keep], g_ewald, eta)
    for a in np.nonzero((flags[:ntotal] & 1) != 0)[0]:
        t = np.zeros(0, dtype=LD)
        if own_row[a] >= 0:
            js = lst.neigh[lst.first[a]:lst.first[a] + lst.numneigh[a]].astype(np.int64) & NEIGHMASK
            t = terms(np.full(len(js), a), js, js)
        owners = tr_entry[tr_ptr[a]:tr_ptr[a + 1]].astype(np.int64) & NEIGHMASK
        t = np.concatenate([t, terms(owners, np.full(len(owners), a), owners)])
        pot[a], A[a] = t.sum(), np.abs(t).sum()
    return pot, A


def pair_direct(x_owned, q_owned, typ_owned, flags_owned, boxlo, prd, periodic, cutsq, cut_coulsq, g_ewald, eta):
    """per selected owned atom the sum over every image of every owned atom (its own images too, itself not): no list, no ghosts.
    An image's coordinates are formed in float64, x + shift * prd, as conp_amd.neighbor.make_ghosts forms a ghost's: the same bits"""
    x64 = np.asarray(x_owned, dtype=np.float64)
    x, q, flags = x64.astype(LD), np.asarray(q_owned, dtype=LD), np.asarray(flags_owned)
    n = len(q)
    rc = float(np.sqrt(min(float(np.max(cutsq)), cut_coulsq)))
    ranges = [range(-int(np.ceil(rc / prd[c])), int(np.ceil(rc / prd[c])) + 1) if periodic[c] else range(1) for c in range(3)]
    eb = (flags >> 1) & 1
    cs = np.asarray(cutsq)
    pot, A = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    for a in np.nonzero((flags & 1) != 0)[0]:
        for sh in itertools.product(*ranges):
            d = x[a] - (x64 + np.array(sh) * np.asarray(prd, dtype=np.float64)).astype(LD)
            rsq = np.maximum((d * d).sum(axis=1), RSQ_FLOOR)
            keep = (rsq < cs[typ_owned[a], typ_owned].astype(LD)) & (rsq < LD(cut_coulsq)) & (q != 0)
            if sh == (0, 0, 0):
                keep[a] = False
            t = q[keep] * dudq_of(rsq[keep], (eb[a] + eb)[keep], g_ewald, eta)
            pot[a] += t.sum(); A[a] += np.abs(t).sum()
    return pot, A


def fold(v, owner, nlocal):
    """ghost rows added onto their owners (owner [nall]: the owning local index of every row)"""
    out = np.array(v[:nlocal], copy=True)
    np.add.at(out, np.asarray(owner)[nlocal:len(v)], v[nlocal:])
    return out


def finish(pair, u, q, z, etabit, eta, slabflag, qsumflag, volume, Q, M, evs):
    """pot = (((pair - u) + [eta bit] eta q sqrt(2) / sqrt(pi)) + z slabcorr) - [qsumflag] (2 pi / V) Q z^2, times evs; with
    slabcorr = 2 (2 pi / V) M (compute_potential_atom.cpp:165-175, :323-345, :214)"""
    pair, u, q, z = (np.asarray(v, dtype=LD) for v in (pair, u, q, z))
    p = pair - u
    if eta != 0.0:
        p = p + np.where(np.asarray(etabit) != 0, LD(eta) * q * SQRT2 / PIS, LD(0))
    if slabflag:
        pi2vol = 2 * LD(np.pi) / LD(volume)
        p = p + z * (2 * pi2vol * LD(M))
        if qsumflag:
            p = p - pi2vol * LD(Q) * z * z
    return p * LD(evs)
