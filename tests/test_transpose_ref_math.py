"""no GPU: the numpy restatement of the transposed half list (tests/transpose_ref.py) against a plain loop, and the crafted list the
GPU tests upload: it really has the rows and segments the kernels can go wrong on, so those tests cannot pass by missing an edge."""
import numpy as np

import transpose_ref as tr


def test_the_crafted_list_has_every_edge():
    far = np.random.default_rng(1).normal(size=(1299, 3))
    for nall, targets in ((401, None), (1299, None), (1299, tr.central_targets(far, 128))):
        lst = tr.crafted_list(nall, targets=targets)
        rows, segs = tr.segment_lengths(lst, nall)
        for k in tr.EDGES:
            assert np.any(rows == k), ("own row", k)
            assert np.any(segs == k), ("transposed segment", k)
        assert rows.max() >= 300 and segs.max() >= 300
        assert np.any((rows < 0) & (segs > 0))                      # a transposed segment, no own row
        assert np.any((rows > 0) & (segs == 0))                     # and the reverse
        assert rows[tr.NEVER_J] > 0 and segs[tr.NEVER_J] == 0
        # an owner missing from ilist: its numneigh / first entries are there, no ilist entry reaches them
        assert tr.MISSING not in lst.ilist and lst.numneigh[tr.MISSING] > 0 and rows[tr.MISSING] == -1
        assert segs.sum() == lst.numneigh[lst.ilist].sum() < lst.neigh.size
        # rows lie in the flat array in non-ascending `first`, in ilist order and in owner order
        assert np.any(np.diff(lst.first[lst.ilist]) < 0) and np.any(np.diff(lst.first[np.sort(lst.ilist)]) < 0)
        assert nall % 4 != 0 and lst.inum % 4 != 0
        assert len(np.unique(lst.ilist)) == lst.inum                # no owner twice
        i, p, raw = tr.slots_of(lst)
        assert np.all((raw & tr.MASK) != i) and np.all((raw & tr.MASK) < nall)
        assert {0, 1, 2, 3} == set(np.unique(raw >> 30))


def test_the_numpy_index_is_the_definition():
    """own_row, tr_ptr and tr_entry by the plain loop of the definition: listed slots in ascending slot order, appended to their j"""
    nall = 401
    lst = tr.crafted_list(nall)
    own_row, tr_ptr, tr_entry = tr.transpose(lst, nall)
    slot_owner = {}
    for ii, i in enumerate(lst.ilist):
        assert own_row[i] == ii
        for p in range(lst.first[i], lst.first[i] + lst.numneigh[i]):
            assert p not in slot_owner                              # rows do not overlap
            slot_owner[p] = int(i)
    assert np.count_nonzero(own_row >= 0) == lst.inum
    seg = [[] for _ in range(nall)]
    for p in sorted(slot_owner):
        raw = int(lst.neigh[p]) & 0xFFFFFFFF
        seg[raw & tr.MASK].append(slot_owner[p] | (raw & 0xC0000000))
    assert tr_ptr[0] == 0 and tr_ptr[-1] == len(slot_owner) and tr_ptr.dtype == np.int32 and tr_entry.dtype == np.int32
    for a in range(nall):
        got = tr_entry[tr_ptr[a]:tr_ptr[a + 1]].astype(np.int64) & 0xFFFFFFFF
        assert list(got) == seg[a], a


def test_a_built_style_list():
    """ilist = 0 .. n-1 with rows in owner order (what the device build leaves): entries of a segment ascend by owner"""
    rng = np.random.default_rng(0)
    n, nall = 50, 80
    numneigh = np.zeros(nall, np.int32)
    numneigh[:n] = rng.integers(0, 9, n)
    first = np.zeros(nall, np.int32)
    first[:n] = np.cumsum(numneigh[:n]) - numneigh[:n]
    neigh = rng.integers(0, nall, numneigh.sum()).astype(np.int32)
    lst = tr.NeighList(inum=n, ilist=np.arange(n, dtype=np.int32), numneigh=numneigh, first=first, neigh=neigh)
    own_row, tr_ptr, tr_entry = tr.transpose(lst, nall)
    assert np.all(own_row[:n] == np.arange(n)) and np.all(own_row[n:] == -1)
    for a in range(nall):
        assert np.all(np.diff(tr_entry[tr_ptr[a]:tr_ptr[a + 1]]) >= 0)
    assert np.all(np.bincount(neigh, minlength=nall) == np.diff(tr_ptr))
