"""numpy reference of the half list conp_pair_build_list_device builds (include/conp_hip.h), and the inputs the
GPU tests use.  The pairs are conp_amd/neighbor.py::_half_pairs; the special-bond bits are restated here from the header:
`which` = class of the FIRST position of tag[j] in special[i][0 .. nspecial[i][2]); the bits are stored when which > 0, the class's
factors are not both 1.0 and no periodic dimension has |del_c| > prd_half[c].  tests/test_neigh_ref_math.py checks this module
without a GPU."""
import functools
from types import SimpleNamespace

import numpy as np

import pair_force_ref as pref
from conp_amd import neighbor
from test_gpu_pair_forces import system

MAXSPECIAL = 8


@functools.lru_cache(maxsize=None)
def inputs(kind, newton):
    """(system, atoms with ghosts, cutneigh, prd_half) of a test case.  small127: `small` without its last owned atom (and that atom's
    images): 127 owners, a ragged last workgroup of the row kernel"""
    base = "small" if kind == "small127" else kind
    s = system(base, newton)
    at = neighbor.make_ghosts(s)
    if kind == "small127":
        keep = np.nonzero(at.owner != at.nlocal - 1)[0]
        at = neighbor.Atoms(nlocal=at.nlocal - 1, nghost=len(keep) - (at.nlocal - 1), x=np.ascontiguousarray(at.x[keep]), q=at.q[keep].copy(),
                            type=at.type[keep].copy(), tag=at.tag[keep].copy(), echeck=at.echeck[keep].copy(), owner=at.owner[keep].copy())
    prd_half = np.where(np.asarray(s.periodic), 0.5 * np.asarray(s.prd, dtype=np.float64), 0.0)
    return SimpleNamespace(kind=kind, newton=newton, s=s, at=at, cutneigh=float(s.cutoff + s.skin), prd_half=prd_half)


def chain_specials(at):
    """LAMMPS' per-atom special tables for a chain over the owned electrolyte atoms in tag order, whatever their distance: k - k+-1 are
    1-2, k - k+-2 1-3, k - k+-3 1-4 partners.  -> (nspecial [nlocal][3] cumulative, special [nlocal][MAXSPECIAL] tags).  Every row with
    a 1-2 partner repeats that partner's tag at the end of its 1-4 block (the first match decides the class), and the slots behind
    nspecial[i][2] hold a 1-3 partner's tag again (they are not searched)."""
    n = at.nlocal
    el = np.nonzero(at.echeck[:n] == 0)[0]
    el = el[np.argsort(at.tag[el], kind="stable")]
    nspecial = np.zeros((n, 3), dtype=np.int32)
    special = np.zeros((n, MAXSPECIAL), dtype=np.int32)
    for k, i in enumerate(el):
        cls = [[at.tag[el[m]] for m in (k - d, k + d) if 0 <= m < len(el)] for d in (1, 2, 3)]
        if cls[0]:
            cls[2].append(cls[0][0])
        row = cls[0] + cls[1] + cls[2]
        assert len(row) < MAXSPECIAL
        nspecial[i] = np.cumsum([len(c) for c in cls])
        special[i, :len(row)] = row
        special[i, len(row):] = cls[1][0] if cls[1] else 0
    return nspecial, special


def special_bits(at, i, j, nspecial, special, special_lj, special_coul, prd_half):
    """which << 30 (int64) for the pairs (i, j), by the rule of the header"""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    tj = at.tag[j]
    n1, n2, n3 = (nspecial[i, c].astype(np.int64) for c in range(3))
    k = np.arange(special.shape[1])[None, :]
    hit = (special[i] == tj[:, None]) & (k < n3[:, None])
    pos = np.where(hit.any(axis=1), hit.argmax(axis=1), -1)                 # first position, -1: absent
    which = np.where(pos < 0, 0, 1 + (pos >= n1) + (pos >= n2))
    flagged = np.array([False] + [not (special_lj[c] == 1.0 and special_coul[c] == 1.0) for c in (1, 2, 3)])
    d = np.abs(at.x[i] - at.x[j])
    ph = np.asarray(prd_half, dtype=np.float64)
    image = ((ph[None, :] > 0) & (d > ph[None, :])).any(axis=1)
    keep = (which > 0) & flagged[which] & ~image
    return np.where(keep, which, 0).astype(np.int64) << 30, SimpleNamespace(which=which, image=image, flagged=flagged[which])


def sort_rows(nlocal, numneigh, neigh):
    """entries sorted inside every row of a list whose rows 0 .. nlocal-1 follow each other in `neigh` (by their unsigned value:
    bits included)"""
    row = np.repeat(np.arange(nlocal), numneigh[:nlocal])
    u = neigh.astype(np.int64) & 0xFFFFFFFF
    return neigh[np.lexsort((u, row))]


def reference(inp, specials=None, special_lj=pref.ONES, special_coul=pref.ONES):
    """the list of the header as a neighbor.NeighList with every row sorted (sort_rows); specials: (nspecial, special) or None"""
    at = inp.at
    p = getattr(inp, "_pairs", None)              # (formed once per input: the il_onelayer deck has 2.7 million)
    if p is None:
        p = inp._pairs = neighbor._half_pairs(at, np.arange(at.nall, dtype=np.int64), None, inp.cutneigh, inp.newton)
    i, j = p[:, 0].astype(np.int64), p[:, 1].astype(np.int64)
    assert np.all(i < at.nlocal) and np.all(i != j)
    entry = j.copy()
    detail = None
    if specials is not None:
        bits, detail = special_bits(at, i, j, specials[0], specials[1], special_lj, special_coul, inp.prd_half)
        entry = j | bits
    order = np.lexsort((entry, i))
    i, entry = i[order], entry[order]
    numneigh = np.bincount(i, minlength=at.nall).astype(np.int32)
    first = np.zeros(at.nall, dtype=np.int32)
    first[:at.nlocal] = (np.cumsum(numneigh[:at.nlocal]) - numneigh[:at.nlocal]).astype(np.int32)
    neigh = np.ascontiguousarray(entry.astype(np.uint32).view(np.int32))
    lst = neighbor.NeighList(inum=at.nlocal, ilist=np.arange(at.nlocal, dtype=np.int32), numneigh=numneigh, first=first, neigh=neigh)
    return lst, SimpleNamespace(i=i, entry=entry, detail=detail, order=order)


def cutoff_margin(inp):
    """smallest | r - cutneigh | over the pairs with an owned member: far above rounding, or `<` against `<=` could change a list"""
    from scipy.spatial import cKDTree
    at, rc = inp.at, inp.cutneigh
    t = cKDTree(at.x)
    near = t.query_pairs(rc + 1e-3, output_type="ndarray")
    near = near[(near[:, 0] < at.nlocal) | (near[:, 1] < at.nlocal)]
    r = np.sqrt(((at.x[near[:, 0]] - at.x[near[:, 1]]) ** 2).sum(axis=1))
    return float(np.abs(r - rc).min())
