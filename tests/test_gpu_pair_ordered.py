"""-m gpu: conp_pair_compute_ordered_device -- the pair forces without a float atomic.

Determinism: three calls on each of two fresh handles agree in every byte of d_f (ghost rows included), d_ev, d_eatom and d_vatom.
Accuracy: the longdouble reference of tests/pair_force_ref.py within the bound of tests/test_gpu_pair_forces.py (1e-12 of the
cancellation-free magnitudes; not a new bound).  Exact cross-check: on a list of disjoint dimers every atom has one term, so the
ordered and the atomic entry must agree in every byte -- this pins the sign, the owner's orientation, the type-row order and the
rule of who receives.  d_ev: byte-equal to the atomic entry's on every case.  The crafted list of tests/transpose_ref.py with real
coordinates: rows and segments at the 64 / 128 edges, an atom count that is no multiple of 4.  Rows of atoms in no listed pair keep a
NaN pre-fill, ghost rows too with newton off.  A whole step on one stream with the ordered entries."""
import functools
import itertools

import numpy as np
import pytest

import pair_force_ref as pref
import transpose_ref as tr
from conp_amd import FixConp
from conp_amd.neighbor import NeighList
from test_gpu_pair_forces import _frac, TOL, case, check

pytestmark = pytest.mark.gpu
NAMES = ("f", "ev", "eatom", "vatom")


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()
    return t


def fresh(c, lst=None):
    """a new handle set up like test_gpu_pair_forces.case's, holding `lst` (default: the case's) and its transposed index"""
    lst = c.lst if lst is None else lst
    fx = FixConp(c.s)
    fx.init_lists(c.lst, c.lst)
    fx.setup_post_neighbor(c.at)
    fx.pair_set_params(c.p.cutsq, c.p.cut_coul, c.p.lj, c.sl, c.sc)
    fx.pair_set_list(lst, c.at.nall)
    fx.pair_transpose_list_device()
    return fx


def call(fx, c, on=NAMES, pre=None, fill=float("nan"), atomic=False, times=1):
    """`times` calls of the ordered (or the atomic) entry with fresh outputs each -> list of dicts name -> numpy array.  d_f starts as
    `pre` (zeros by default), the overwritten outputs as `fill`."""
    import torch
    nall = c.at.nall
    d_x, d_q = _dev(c.at.x.astype(np.float64)), _dev(c.at.q.astype(np.float64))
    shapes = dict(f=(nall, 3), ev=(8,), eatom=(nall,), vatom=(nall, 6))
    entry = fx.pair_compute_device if atomic else fx.pair_compute_ordered_device
    outs = []
    for _ in range(times):
        t = {m: (_dev(np.zeros(shapes["f"]) if pre is None else pre.copy()) if m == "f" else
                 torch.full(shapes[m], fill, dtype=torch.float64, device="cuda")) for m in on}
        torch.cuda.synchronize()
        entry(d_x.data_ptr(), d_q.data_ptr(), *[t[m].data_ptr() if m in t else 0 for m in NAMES])
        outs.append(t)
    torch.cuda.synchronize()
    return [{m: v.cpu().numpy() for m, v in t.items()} for t in outs]


def as_check(o):
    ev = o.get("ev")
    return o.get("f"), (None if ev is None else ev[:2]), (None if ev is None else ev[2:]), o.get("eatom"), o.get("vatom")


def same_bytes(outs, tag):
    for o in outs[1:]:
        for m in outs[0]:
            assert o[m].tobytes() == outs[0][m].tobytes(), (tag, m)


def deterministic_and_right(c, R, tag, lst=None, on=NAMES):
    """three calls on each of two fresh handles: every byte equal; the reference's bound; d_ev byte-equal to the atomic entry's"""
    pre = np.random.default_rng(7).normal(size=(c.at.nall, 3))
    outs, zero = [], None
    for _ in range(2):
        fx = fresh(c, lst)
        outs += call(fx, c, on=on, pre=pre, times=3)
        if zero is None:
            zero = call(fx, c, on=on)[0]
            if "ev" in on:
                atomic = call(fx, c, on=on, atomic=True)[0]
                assert zero["ev"].tobytes() == atomic["ev"].tobytes(), (tag, "d_ev against the atomic entry")
        fx.close()
    same_bytes(outs, tag)
    if "ev" in on:
        assert outs[0]["ev"].tobytes() == zero["ev"].tobytes(), tag
    check(tag, as_check(zero), R)
    if "f" in on:                                                    # pre-fill + force: one more rounding, of the sum
        slack = 4e-16 * (np.abs(pre) + np.abs(R.f.astype(float)))
        assert _frac(tag + ": pre-filled f", outs[0]["f"] - pre, R.f, TOL * R.A[:, None] + slack) <= 1.0
    return outs[0], zero


@pytest.mark.parametrize("kind,newton,special,lj", [
    ("small", False, False, True), ("small", True, False, True), ("sparse", True, False, True), ("sparse", False, False, True),
    ("il_onelayer", False, False, True), ("small", False, True, True), ("small", True, True, True), ("small", True, False, False),
    ("manytypes", True, False, True), ("manytypes", False, False, True)])
def test_deterministic_and_within_the_bound(kind, newton, special, lj):
    c = case(kind, newton, special=special, lj=lj)
    if kind == "manytypes":
        assert (c.s.ntypes + 1) ** 2 > 256                          # the table is read from global memory
    pre_out, zero = deterministic_and_right(c, c.R, c.tag + ("" if lj else ", no LJ part") + " (ordered)")
    n = c.at.nlocal
    if not newton:                                                   # no ghost row is written
        assert np.all(zero["f"][n:] == 0) and np.all(zero["eatom"][n:] == 0) and np.all(zero["vatom"][n:] == 0)
    else:
        assert np.abs(zero["f"][n:]).max() > 0


@pytest.mark.parametrize("on", [s for k in range(1, 5) for s in itertools.combinations(NAMES, k)], ids="+".join)
def test_every_combination_of_null_outputs(on):
    c = case("small", True)
    fx = case("small", True).fx
    fx.pair_set_list(c.lst, c.at.nall)
    fx.pair_transpose_list_device()
    pre = np.random.default_rng(8).normal(size=(c.at.nall, 3))
    outs = call(fx, c, on=on, pre=pre, times=3) + call(fresh_shared(), c, on=on, pre=pre, times=3)
    same_bytes(outs, "+".join(on))
    zero = call(fx, c, on=on)[0]
    check("outputs " + "+".join(on), as_check(zero), c.R)
    if "ev" in on:
        assert zero["ev"].tobytes() == call(fx, c, on=on, atomic=True)[0]["ev"].tobytes()


@functools.lru_cache(maxsize=None)
def fresh_shared():
    """the second handle of the NULL-output cases (one for all fifteen: the entry keeps no state between calls)"""
    return fresh(case("small", True))


def test_all_outputs_null():
    c = case("small", True)
    fx = fresh_shared()
    d_x, d_q = _dev(c.at.x), _dev(c.at.q)
    fx.pair_compute_ordered_device(d_x.data_ptr(), d_q.data_ptr(), 0, 0, 0, 0)       # CONP_OK (anything else raises)


# ---- the exact cross-check -----------------------------------------------------------------------------------------------------------
def dimers(c, seed=3):
    """disjoint listed pairs of the case's list (every atom in at most one), in a shuffled order, a third with special bits"""
    i, jraw = pref.pairs_of(c.lst)
    j = jraw & pref.NEIGHMASK
    rng = np.random.default_rng(seed)
    used = np.zeros(c.at.nall, bool)
    rows = []
    for k in rng.permutation(len(i)):
        if not used[i[k]] and not used[j[k]] and i[k] != j[k]:
            used[i[k]] = used[j[k]] = True
            a, b = (int(j[k]), int(i[k])) if j[k] < c.at.nlocal and rng.random() < 0.5 else (int(i[k]), int(j[k]))   # both orientations
            rows.append((a, b | (int(rng.integers(1, 4)) << 30 if rng.random() < 0.33 else 0)))
    nall = c.at.nall
    numneigh, first = np.zeros(nall, np.int32), np.zeros(nall, np.int32)
    for k, (a, _) in enumerate(rows):
        numneigh[a], first[a] = 1, k
    lst = NeighList(inum=len(rows), ilist=np.array([a for a, _ in rows], np.int32), numneigh=numneigh, first=first,
                    neigh=np.array([b for _, b in rows], np.int64).astype(np.uint32).view(np.int32))
    return lst, used


@pytest.mark.parametrize("newton", [False, True])
def test_disjoint_dimers_agree_with_the_atomic_entry_in_every_byte(newton):
    c = case("small", newton, special=True)
    lst, used = dimers(c)
    n = c.at.nlocal
    i, jraw = pref.pairs_of(lst)
    j = jraw & pref.NEIGHMASK
    assert lst.inum > 20 and np.any(i < j) and np.any(i > j) and np.any(j >= n) and np.any(j < n) and np.any(jraw >> 30)
    assert np.bincount(np.concatenate([i, j]), minlength=c.at.nall).max() == 1
    fx = fresh(c, lst)
    rng = np.random.default_rng(12)
    pre = rng.normal(size=(c.at.nall, 3)) + 3.0 * np.sign(rng.normal(size=(c.at.nall, 3)))      # no zero, no tiny entry
    o = call(fx, c, pre=pre, fill=1.25)[0]
    a = call(fx, c, pre=pre, fill=1.25, atomic=True)[0]
    for m in NAMES:
        assert o[m].tobytes() == a[m].tobytes(), m
    R = pref.for_atoms(c.at, lst, c.p, c.s, newton, c.sl, c.sc)
    assert np.abs(o["f"] - pre).max() > 1.0 and R.npairs > 10
    # rows of atoms in no listed pair keep a NaN pre-fill; with newton off so do the ghost rows
    nan = np.full((c.at.nall, 3), np.nan)
    o = call(fx, c, on=("f",), pre=nan)[0]["f"]
    a = call(fx, c, on=("f",), pre=nan, atomic=True)[0]["f"]
    assert np.array_equal(np.isnan(o), np.isnan(a))
    assert np.all(np.isnan(o[~used])) and np.any(~used)
    if not newton:
        assert np.all(np.isnan(o[n:]))
    fx.close()


# ---- the crafted list with real coordinates --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("newton", [False, True])
def test_the_crafted_list_with_real_coordinates(newton):
    c = case("small", newton, special=True)
    nall, n = c.at.nall, c.at.nlocal
    assert nall % 4 != 0
    targets = tr.central_targets(c.at.x, n)                         # the j-only atoms lie among the owned ones: their pairs act
    lst = tr.crafted_list(nall, targets=targets)
    R = pref.for_atoms(c.at, lst, c.p, c.s, newton, c.sl, c.sc)
    assert R.rmin >= 0.8
    # the 300-entry row and the 310-entry segment hold several terms inside the cutoff: sums with an order to get wrong
    assert np.count_nonzero(R.i == tr.N_TARGET - 1) >= 8 and np.count_nonzero(R.j == targets[-1]) >= 8
    filled, zero = deterministic_and_right(c, R, f"crafted list, newton {'on' if newton else 'off'}", lst=lst)
    # untouched rows keep their bytes -- a random pre-fill and a NaN pre-fill -- where no listed pair names the atom, and on ghost
    # rows with newton off; rows with terms change
    rows, segs = tr.segment_lengths(lst, nall)
    untouched = (rows <= 0) & (segs == 0)
    if not newton:
        untouched[n:] = True
    assert untouched[targets[0]]                                    # (named by no slot, owns no row)
    pre = np.random.default_rng(7).normal(size=(nall, 3))           # (deterministic_and_right's pre-fill)
    assert filled["f"][untouched].tobytes() == pre[untouched].tobytes()
    acted = np.abs(R.f.astype(float)).max(axis=1) > 1e-6
    assert np.all(np.any(filled["f"][acted] != pre[acted], axis=1)) and not np.any(acted & untouched)
    fx = fresh(c, lst)
    f = call(fx, c, on=("f",), pre=np.full((nall, 3), np.nan))[0]["f"]
    assert np.all(np.isnan(f[untouched]))
    fx.close()


# ---- a whole step on one stream ---------------------------------------------------------------------------------------------------------
def test_a_whole_step_with_nothing_between():
    """pre_force_device -> ewald_forces_device -> pair_compute_ordered_device -> post_force_ordered_device -> ghost_fold_device on
    one stream, one synchronisation: tests/test_gpu_post_force_device.py's whole step with the two ordered entries, held to the sum
    of the three host entries folded in numpy, to that test's bound (1e-9 of the largest entry: the loosest of the three)"""
    import torch
    import test_gpu_post_neighbor_device as tp
    from helpers import rel_err
    from test_gpu_post_force_device import ORACLE, _device_and_host_handles
    c, fd, fh, b, d_q = _device_and_host_handles(True)
    n, nall = b.n, b.nall
    p = pref.lj_tables(c.s.ntypes, c.s.cutoff)
    fd.pair_set_params(p.cutsq, p.cut_coul, None); fh.pair_set_params(p.cutsq, p.cut_coul, None)
    fd.pair_transpose_list_device()
    fd.fix_transpose_list_device()
    d_f = torch.zeros((nall, 3), dtype=torch.float64, device="cuda")
    d_out = torch.full((9,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    fd.pre_force_device(b.d_x.data_ptr(), d_q.data_ptr(), c.s.potdiff)
    fd.ewald_forces_device(b.d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), 0, 0)
    fd.pair_compute_ordered_device(b.d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), 0, 0, 0)
    fd.post_force_ordered_device(b.d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), d_out.data_ptr())
    fd.ghost_fold_device(d_f.data_ptr(), 3)
    torch.cuda.synchronize()
    got = d_f.cpu().numpy()[:n]
    at1, lst = tp.host_route(fh, c, fd, b)
    at1.q[:] = d_q.cpu().numpy()[:nall]
    fh.pair_set_list(lst, nall)
    total = np.zeros((nall, 3))
    total[:n] += fh.ewald_forces(at1, energy=False, virial=False)[0]
    total += fh.pair_compute(at1, eng=False, virial=False, eatom=False, vatom=False)[0]
    f_post = fh.post_force(at1)[0]
    total += f_post
    assert np.abs(f_post).max() > 0 and np.any(f_post[n:] != 0.0) and d_out.cpu().numpy()[8] > 0   # the term acted, on ghost rows too
    owner = np.asarray(fd.ghost_get()[2], np.int64)
    want = total[:n].copy()
    np.add.at(want, owner, total[n:])
    fr = rel_err(got, want) / ORACLE
    print(f"a whole step with the ordered entries: fraction of the bound {ORACLE:g}: force {fr:.3g}")
    assert fr < 1.0
    without = (total - f_post)[:n].copy()
    np.add.at(without, owner, (total - f_post)[n:])
    assert rel_err(got, without) > 1e3 * ORACLE                        # ... and the sum without the Gaussian term is far outside
    fd.close(); fh.close()
