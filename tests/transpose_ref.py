"""The transposed half list of DESIGN.md section 26 restated in numpy (a stable argsort of the listed slots by j), and the crafted
list the GPU tests of the index and of the atomic-free entries share: rows and transposed segments at every wave edge."""
import numpy as np

from conp_amd.neighbor import NeighList

MASK = 0x3FFFFFFF
EDGES = (0, 1, 63, 64, 65, 127, 128, 129)      # lengths around one and two passes of a 64-lane loop
LONG_ROW, LONG_SEG = 300, 310                   # "a few hundred": several passes, a ragged last one
N_OWN = 340                                     # atoms 0 .. N_OWN-1 may own a row
MISSING = 17                                    # has numneigh / first entries but is not in ilist
NEVER_J = 5                                     # owns a row, is nobody's j
N_TARGET = len(EDGES) + 1                       # atoms that are j only, with prescribed segment lengths


def slots_of(lst):
    """(i, p, raw) of every listed slot in ascending slot order p"""
    own = np.asarray(lst.ilist[:lst.inum], dtype=np.int64)
    cnt = lst.numneigh[own].astype(np.int64)
    i = np.repeat(own, cnt)
    p = np.repeat(lst.first[own].astype(np.int64), cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    o = np.argsort(p, kind="stable")
    i, p = i[o], p[o]
    return i, p, lst.neigh[p].astype(np.int64) & 0xFFFFFFFF


def transpose(lst, nall):
    """-> (own_row [nall], tr_ptr [nall + 1], tr_entry [listed slots]) int32"""
    own_row = np.full(nall, -1, dtype=np.int32)
    own_row[lst.ilist[:lst.inum]] = np.arange(lst.inum, dtype=np.int32)
    i, p, raw = slots_of(lst)
    j = raw & MASK
    o = np.argsort(j, kind="stable")                # slots of one j keep ascending p
    entry = (i | (raw & 0xC0000000))[o]
    tr_ptr = np.zeros(nall + 1, dtype=np.int64)
    np.cumsum(np.bincount(j, minlength=nall), out=tr_ptr[1:])
    return own_row, tr_ptr.astype(np.int32), entry.astype(np.uint32).view(np.int32)


def segment_lengths(lst, nall):
    own_row, tr_ptr, _ = transpose(lst, nall)
    rows = np.where(own_row >= 0, lst.numneigh[:nall], -1)          # -1: no own row
    return rows, np.diff(tr_ptr)


def central_targets(x, nlocal):
    """N_TARGET atoms that own no row (index >= N_OWN), those closest to the centroid of the owned atoms: with real coordinates
    their transposed segments then hold pairs inside the cutoff"""
    d = np.linalg.norm(np.asarray(x, np.float64)[N_OWN:] - np.asarray(x, np.float64)[:nlocal].mean(axis=0), axis=1)
    return np.sort(N_OWN + np.argsort(d, kind="stable")[:N_TARGET])


def crafted_list(nall=401, seed=11, targets=None):
    """A half list over nall >= 401 atoms (any index below nall is a valid list; i == j never occurs, so it can be run with real
    coordinates).  Owners 0 .. 8 have rows of EDGES + (LONG_ROW,) entries, the nine `targets` (default: the last nine atoms) are
    named by exactly EDGES + (LONG_SEG,) slots and own nothing; atom NEVER_J owns a row and is nobody's j; atom MISSING has
    numneigh / first entries that no ilist entry reaches; the rows lie in the flat array in a shuffled order with gaps, ilist is shuffled, a fifth of the entries
    carry special bits."""
    assert nall >= N_OWN + N_TARGET + 40
    rng = np.random.default_rng(seed)
    targets = np.arange(nall - N_TARGET, nall) if targets is None else np.asarray(targets)
    assert len(targets) == N_TARGET and targets.min() >= N_OWN and targets.max() < nall and len(set(targets)) == N_TARGET
    fixed = dict(zip(range(N_TARGET), EDGES + (LONG_ROW,)))
    owners = [o for o in range(N_OWN) if o != MISSING]
    free = [o for o in owners if o not in fixed]                      # owners whose rows take the targets' slots
    pool = np.array([a for a in range(nall) if a != NEVER_J and a not in set(int(t) for t in targets)])
    rows = {o: [] for o in owners}
    for t, k in zip(targets, EDGES + (LONG_SEG,)):
        for o in rng.choice(free, size=k, replace=False):
            rows[o].append(int(t))
    for o in owners:
        want = fixed[o] if o in fixed else len(rows[o]) + int(rng.integers(0, 30))
        cand = pool[pool != o]
        rows[o] += [int(v) for v in rng.choice(cand, size=want - len(rows[o]), replace=True)]
        rng.shuffle(rows[o])
    rows[MISSING] = [int(v) for v in rng.choice(pool[pool != MISSING], size=5)]
    numneigh, first = np.zeros(nall, np.int32), np.zeros(nall, np.int32)
    flat = []
    for o in rng.permutation(list(rows)):
        flat += [0] * int(rng.integers(0, 3))                         # a gap no row owns
        first[o], numneigh[o] = len(flat), len(rows[o])
        flat += rows[o]
    neigh = np.array(flat, dtype=np.int64)
    bits = np.where(rng.random(neigh.size) < 0.2, rng.integers(1, 4, neigh.size), 0)
    neigh = (neigh | (bits << 30)).astype(np.uint32).view(np.int32)
    ilist = rng.permutation(np.array(owners, dtype=np.int32)).astype(np.int32)
    return NeighList(inum=len(owners), ilist=np.ascontiguousarray(ilist), numneigh=numneigh, first=first, neigh=np.ascontiguousarray(neigh))
