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
