"""numpy reference of the ghost entries of include/conp_hip.h: conp_ghost_build_device, conp_ghost_fill_device,
conp_ghost_fold_device and conp_atoms_wrap_device, restated from the header -- not through conp_amd/neighbor.py::make_ghosts, which
tests/test_ghost_ref_math.py compares this module with (without a GPU)."""
import itertools
from types import SimpleNamespace

import numpy as np


def box_of(s):
    """(boxlo, boxhi, periodic, cutghost) of a systems.System: cutghost = cutoff + skin, the list cutoff"""
    return np.asarray(s.boxlo, np.float64), np.asarray(s.boxhi, np.float64), tuple(bool(p) for p in s.periodic), float(s.cutoff + s.skin)


def shifts(boxlo, boxhi, periodic, cutghost):
    """the shift triples in the order of the header (sx slowest, sz fastest, ascending, (0, 0, 0) skipped) -> ([nshift][3] int64, prd)"""
    prd = np.asarray(boxhi, np.float64) - np.asarray(boxlo, np.float64)
    m = [int(np.ceil(cutghost / prd[c])) if periodic[c] else 0 for c in range(3)]
    sh = [t for t in itertools.product(*[range(-k, k + 1) for k in m]) if t != (0, 0, 0)]
    return np.array(sh, dtype=np.int64).reshape(len(sh), 3), prd


def build(x, boxlo, boxhi, periodic, cutghost):
    """owner [nghost], img [nghost][3] (int32) in the header's order; x_all [nlocal + nghost][3]; margin: the smallest distance of
    any shifted coordinate of a finite owned coordinate from lo and hi"""
    x = np.asarray(x, np.float64).reshape(-1, 3)
    boxlo, boxhi = np.asarray(boxlo, np.float64), np.asarray(boxhi, np.float64)
    sh, prd = shifts(boxlo, boxhi, periodic, cutghost)
    lo, hi = boxlo - cutghost, boxhi + cutghost
    owner, img, margin = [], [], np.inf
    with np.errstate(invalid="ignore"):
        for s in sh:
            xi = x + (s.astype(np.float64) * prd)          # the product first, then the sum
            keep = np.all((xi >= lo) & (xi < hi), axis=1)
            d = np.minimum(np.abs(xi - lo), np.abs(xi - hi))
            d = d[np.isfinite(d)]
            if d.size:
                margin = min(margin, float(d.min()))
            o = np.nonzero(keep)[0]
            owner.append(o)
            img.append(np.broadcast_to(s, (len(o), 3)))
    owner = np.concatenate(owner).astype(np.int32) if owner else np.zeros(0, np.int32)
    img = np.concatenate(img).astype(np.int32).reshape(len(owner), 3) if img else np.zeros((0, 3), np.int32)
    return SimpleNamespace(nlocal=len(x), nghost=len(owner), owner=owner, img=img, prd=prd, lo=lo, hi=hi, nshift=len(sh), margin=margin,
                           x=fill(x, owner, img, prd))


def fill(x_owned, owner, img, prd):
    """[nlocal + nghost][3]: the owned rows, then x[owner] + img * prd per ghost"""
    x_owned = np.asarray(x_owned, np.float64).reshape(-1, 3)
    return np.ascontiguousarray(np.concatenate([x_owned, x_owned[owner] + (img.astype(np.float64) * prd)]))


def fold(v, owner, nlocal):
    """v [nlocal + nghost][...] -> a copy whose owned rows are (((v[o] + v[g1]) + v[g2]) + ...) over the owner's ghosts in ascending
    ghost index, in v's own precision; ghost rows unchanged.  Round k adds every owner's k-th ghost: each owner's sum is sequential"""
    out = np.array(v, copy=True)
    owner = np.asarray(owner, np.int64)
    order = np.argsort(owner, kind="stable")                # ghosts grouped by owner, ascending ghost index inside a group
    so = owner[order]
    rank = np.arange(len(so)) - np.searchsorted(so, so, side="left")
    for k in range(int(rank.max()) + 1 if len(rank) else 0):
        g = order[rank == k]
        out[owner[g]] = out[owner[g]] + v[nlocal + g]
    return out


def wrap(x, boxlo, boxhi, periodic, image=None):
    """-> (x, image) after the one-pass remap of the header; image: int32 [n][3] counters (zeros when None)"""
    x = np.array(x, dtype=np.float64, copy=True).reshape(-1, 3)
    image = np.zeros(x.shape, np.int32) if image is None else np.array(image, dtype=np.int32, copy=True)
    with np.errstate(invalid="ignore"):
        for c in range(3):
            if not periodic[c]:
                continue
            prd = np.float64(boxhi[c]) - np.float64(boxlo[c])
            below = x[:, c] < boxlo[c]
            x[below, c] = x[below, c] + prd
            image[below, c] -= 1
            above = x[:, c] >= boxhi[c]
            x[above, c] = np.maximum(x[above, c] - prd, boxlo[c])
            image[above, c] += 1
    return x, image


def edge_case():
    """a box and three atoms for the remap's edges: dimension 0 is exact (0 .. 10), dimension 1 a box whose boxhi - prd rounds BELOW
    boxlo (found by a fixed scan), dimension 2 is not periodic.  Atoms: one with x exactly at boxhi, one exactly at boxlo in every
    dimension, one with y exactly at boxhi (it lands below boxlo and is clamped onto it) and z outside its non-periodic bounds."""
    rng = np.random.default_rng(18)
    for _ in range(10000):
        lo1 = float(rng.uniform(-3.0, 3.0))
        hi1 = lo1 + float(rng.uniform(5.0, 30.0))
        prd1 = np.float64(hi1) - np.float64(lo1)
        if np.float64(hi1) - prd1 < lo1:
            break
    else:
        raise AssertionError("no box with boxhi - prd < boxlo found")
    boxlo, boxhi = np.array([0.0, lo1, -4.0]), np.array([10.0, hi1, 4.0])
    x = np.array([[10.0, 0.5 * (lo1 + hi1), 1.0], [0.0, lo1, -4.0], [5.0, hi1, 9.0]])
    want_x = np.array([[0.0, 0.5 * (lo1 + hi1), 1.0], [0.0, lo1, -4.0], [5.0, lo1, 9.0]])
    want_image = np.array([[1, 0, 0], [0, 0, 0], [0, 1, 0]], np.int32)
    return SimpleNamespace(boxlo=boxlo, boxhi=boxhi, periodic=(True, True, False), x=x, want_x=want_x, want_image=want_image)
