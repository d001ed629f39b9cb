"""numpy restatement of what conp_fix_post_neighbor_device rebuilds (include/conp_hip.h) -- the charge scatter
lists (2), the electrolyte list (4), the z-window order (5) and the electrode rows of the real-space b (3) -- from the header's
rules, and the inputs the GPU tests use.  tests/test_post_neighbor_ref_math.py checks this module without a GPU."""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np

import ghost_ref as gref

ZN_W = 15                 # taps of the z window: i0 = ceil(ur - ZN_W / 2)
SMALL = ["small", "small127", "sparse"]
MEDIUM = ["medium", "ragged", "rough"]


# ---- the rules ------------------------------------------------------------------------------------------------------------------------
def rows_of_owned(echeck_owned):
    """atom -> electrode row of the owned atoms of one rank at the first post_neighbor: electrode atoms are numbered in ascending
    local index (fix_conp.cpp:480-535 with one rank), -1 for the others"""
    ele = np.asarray(echeck_owned) != 0
    return np.where(ele, np.cumsum(ele) - 1, -1).astype(np.int32)


def scatter_lists(a2e_owned, owner, ne):
    """(2): ele_pairs [k][2] = (atom, row) of owned and ghost electrode atoms in ascending atom index; the CSR by row: per row the
    owned atom, then its ghosts in ascending ghost index"""
    n = len(a2e_owned)
    a2e = np.concatenate([a2e_owned, np.asarray(a2e_owned)[owner]]).astype(np.int64)
    atoms = np.nonzero(a2e >= 0)[0]
    pairs = np.stack([atoms, a2e[atoms]], axis=1).astype(np.int32).reshape(-1, 2)
    ptr = np.zeros(ne + 1, np.int64)
    np.add.at(ptr, a2e[atoms] + 1, 1)
    ptr = np.cumsum(ptr)
    of, row = [], []
    own_of = {int(a2e_owned[i]): i for i in range(n) if a2e_owned[i] >= 0}
    ghosts_of = {}
    for g, o in enumerate(np.asarray(owner)):
        ghosts_of.setdefault(int(o), []).append(n + g)          # ascending ghost index
    for r in range(ne):
        if r not in own_of:
            continue
        members = [own_of[r]] + ghosts_of.get(own_of[r], [])
        of += members
        row += [r] * len(members)
    return SimpleNamespace(ele_pairs=pairs, csr_ptr=ptr.astype(np.int32), csr_of=np.array(of, np.int32), csr_row=np.array(row, np.int32))


def elyte_list(a2e_owned, q_owned):
    """(4): owned atoms without an electrode row and with q != 0, ascending"""
    return np.nonzero((np.asarray(a2e_owned) < 0) & (np.asarray(q_owned) != 0))[0].astype(np.int32)


def zn_grid(nz):
    """grid cells of the z window for nz = (largest kz of the k tables) + 1"""
    return max(64, (38 * nz // 10 + 15) // 16 * 16)


def z_cells(z, n, lz):
    """(5), first half: u = z gscale; u -= n floor(u (1 / n)); c = (int)u, clamped at n.  numpy float64 evaluates these products and
    sums one by one, as the header demands"""
    z = np.asarray(z, np.float64)
    gscale = np.float64(n) / np.float64(lz)
    rn = np.float64(1.0) / np.float64(n)
    u = z * gscale
    u = u - np.float64(n) * np.floor(u * rn)
    c = u.astype(np.int64)                          # truncation, u >= 0
    top = c >= n
    c[top] = n - 1
    u[top] = np.nextafter(np.float64(n), 0.0)
    return u, c


def start_cell(occ):
    """the cell behind the longest run of empty cells: the ring walked twice from cell 0, strictly-greater keeps the first of equally
    long runs, a run is at most n long; no empty cell: 0"""
    n = len(occ)
    best_len = best_end = run = 0
    for c in range(2 * n):
        if occ[c % n] == 0:
            run += 1
            if run > best_len and run <= n:
                best_len, best_end = run, c % n
        else:
            run = 0
    return (best_end + 1) % n if best_len > 0 else 0


def z_order(z_listed, n, lz):
    """(5): for the listed atoms' z in list order -> the permutation `order` (sorted[k] = list[order[k]]: stable by (c - c0) mod n),
    the chunk bounds of i0 = ceil(ur - 7.5), and `margin`: the smallest distance of any u and any ur - 7.5 from an integer"""
    u, c = z_cells(z_listed, n, lz)
    occ = np.bincount(c, minlength=n)
    c0 = start_cell(occ)
    key = (c - c0) % n
    order = np.argsort(key, kind="stable")
    ur = u - np.float64(c0)
    ur = np.where(ur < 0.0, ur + np.float64(n), ur)
    t = ur - np.float64(0.5 * ZN_W)
    i0 = np.ceil(t).astype(np.int64)
    s = i0[order]
    nch = (len(s) + 15) // 16
    pad = np.full(16 * nch - len(s), s[-1] if len(s) else 0)
    blk = np.concatenate([s, pad]).reshape(nch, 16)
    frac = lambda v: np.abs(v - np.round(v))
    margin = float(min(frac(u).min(), frac(t).min())) if len(u) else np.inf
    return SimpleNamespace(u=u, cell=c, occ=occ, c_start=c0, key=key, order=order, i0=i0, ch_lo=blk.min(axis=1).astype(np.int32),
                           ch_hi=blk.max(axis=1).astype(np.int32), margin=margin)


def b_rows(lst, a2e, nlocal, newton, ne):
    """(3): the pairs of a half list with exactly one electrode member, regrouped by that member's row, list order inside a row
    (blist_coul_cal's membership, fix_conp.cpp:1326-1350): an electrode owner i with a non-electrode neighbour j gives (row of i: i, j);
    a non-electrode owner with an electrode neighbour j gives (row of j: j, i) if newton is on or j is owned"""
    own = np.asarray(lst.ilist[:lst.inum], np.int64)
    cnt = lst.numneigh[own].astype(np.int64)
    i = np.repeat(own, cnt)
    start = np.repeat(lst.first[own].astype(np.int64), cnt)
    within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    j = lst.neigh[start + within].astype(np.int64) & 0x3FFFFFFF
    a2e = np.asarray(a2e, np.int64)
    ri, rj = a2e[i], a2e[j]
    first = (ri >= 0) & (rj < 0)
    second = (ri < 0) & (rj >= 0) & (bool(newton) | (j < nlocal))
    row = np.where(first, ri, np.where(second, rj, -1))
    keep = row >= 0
    ele = np.where(first, i, j)[keep]
    oth = np.where(first, j, i)[keep]
    row = row[keep]
    order = np.argsort(row, kind="stable")
    ptr = np.concatenate([[0], np.cumsum(np.bincount(row, minlength=ne))])
    return SimpleNamespace(b_rowptr=ptr.astype(np.int32), b_ele=ele[order].astype(np.int32), b_oth=oth[order].astype(np.int32))


# ---- the inputs of the GPU tests ------------------------------------------------------------------------------------------------------
def _medium_system(kind):
    from conp_amd import systems
    from test_gpu_zwindow import _medium, _rough
    if kind == "medium":
        s = _medium("ffield")
    elif kind == "rough":
        s = _rough("ffield")
    else:                       # the box of test_z_window_ragged_list_across_the_periodic_wrap
        s = _medium("ffield", seed=19)
        lo, hi = s.boxlo[2], s.boxlo[2] + s.prd[2]
        s.x[:, 2] = lo + np.mod(s.x[:, 2] - lo + 0.37 * s.prd[2], s.prd[2])
        assert s.x[:, 2].min() >= lo and s.x[:, 2].max() < hi
        sol = np.nonzero((s.echeck == 0) & (s.q != 0))[0]
        s.q[sol[[3, 500, 7001, 7002, 16000]]] = 0.0
    return dataclasses.replace(s, eletypes=None)


@functools.lru_cache(maxsize=None)
def case(kind, newton=False, seed=41, cut_extra=0.0):
    """a test case: the system, the owned atoms at setup (x0) and after the move (x1, not yet wrapped), the numpy result of wrap ->
    ghost build -> fill at the moved positions.  Electrolyte atoms move by at most 1 A; three of them are pushed across a periodic
    face in x or y.  `cut_extra` is added to the cutoff of the ghosts and of the list (more ghosts, a longer list).  Electrode atoms stay: the A matrix is the setup's."""
    import neigh_ref as nref
    from test_gpu_pair_forces import system
    if kind in SMALL:
        inp = nref.inputs(kind, newton)
        s, a, n = inp.s, inp.at, inp.at.nlocal
        own = SimpleNamespace(x=a.x[:n].copy(), q=a.q[:n].copy(), type=a.type[:n].copy(), tag=a.tag[:n].copy(), echeck=a.echeck[:n].copy())
    else:
        s = system("il_onelayer", newton) if kind == "il_onelayer" else dataclasses.replace(_medium_system(kind), newton=newton)
        n = s.natoms
        own = SimpleNamespace(x=s.x.copy(), q=s.q.copy(), type=s.type.copy(), tag=s.tag.copy(), echeck=s.echeck.copy())
    boxlo, boxhi, periodic, cut = gref.box_of(s)
    cut += cut_extra
    rng = np.random.default_rng(seed)
    sol = np.nonzero(own.echeck == 0)[0]
    step = rng.uniform(-1.0, 1.0, size=(len(sol), 3))
    step *= rng.uniform(0.0, 1.0, size=(len(sol), 1)) / np.linalg.norm(step, axis=1, keepdims=True)
    x1 = own.x.copy()
    x1[sol] += step
    prd = boxhi - boxlo
    x1[sol[1], 0] = boxhi[0] + 0.3
    x1[sol[5], 1] = boxlo[1] - 0.2
    x1[sol[9], 0] = boxlo[0] - 0.45
    assert np.abs(step).max() <= 1.0 and periodic[0] and periodic[1] and prd.min() > 1.0
    xw, _ = gref.wrap(x1, boxlo, boxhi, periodic)
    g = gref.build(xw, boxlo, boxhi, periodic, cut)
    assert np.any(xw != x1) and g.margin >= 1e-9
    a2e = rows_of_owned(own.echeck)
    return SimpleNamespace(kind=kind, newton=newton, s=s, n=n, own=own, x1=x1, xw=xw, ghosts=g, nall=n + g.nghost, box=(boxlo, boxhi, periodic, cut),
                           cutneigh=cut, a2e=a2e, ne=int((own.echeck != 0).sum()),
                           prd_half=np.where(np.asarray(periodic), 0.5 * prd, 0.0))


def zn_setup(c):
    """(n, lz) of the case's z grid from the host k tables, as Fix::zn_order_list takes them from its plan"""
    from conp_amd import capi
    s = c.s
    sq = dataclasses.replace(s, q=c.own.q, tag=c.own.tag) if c.n != s.natoms else s
    kt = capi.host_ktables(sq)
    n = zn_grid(int(kt["kcount_dims"][2]) + 1)
    lz = float(s.prd[2]) * (s.slab_volfactor if s.slabflag else 1.0)
    return n, lz


def expected(c):
    """the tables of the header for a case at its moved, wrapped positions (without the b rows, which need the list)"""
    sc = scatter_lists(c.a2e, c.ghosts.owner, c.ne)
    el = elyte_list(c.a2e, c.own.q)
    return SimpleNamespace(elyte=el, **vars(sc))
