"""-m gpu: conp_pair_compute -- the lj/cut/coul/long pair loop on the device against the longdouble reference of
tests/pair_force_ref.py (itself checked by tests/test_pair_force_math.py).

Bounds (cancellation-free magnitudes of the reference): per atom and component |f_i - ref_i| <= 1e-12 A_i -- a term carries a few tens
of ulp (exp, the polynomial's cancellation, two divisions), a row sums fewer than 1000 terms (<= 1.1e-13 worst case), so 1e-12 leaves
about a tenfold margin; energy and virial entries 1e-12 of E_abs / W_abs; eatom / vatom entries 1e-12 of their per-atom magnitude sums.

Inputs: systems.small_random(ne_side=4, n_elyte=64, seed 4) -- rows of 144-352 neighbours (newton off), 38-253 (newton on), smallest
distance 0.815 A; the il_onelayer deck; and, because no atom of those two can have an empty row (every atom sees its own periodic
images), the same small box stretched to lz = 200 with cutoff 6 in slab geometry, whose newton-on list has rows of 0-56 neighbours."""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import pair_force_ref as pref
from conp_amd import ConpError, FixConp, neighbor, systems
from conp_amd import capi

pytestmark = pytest.mark.gpu
TOL = 1e-12


def system(kind, newton):
    if kind == "small":
        s = systems.small_random(ne_side=4, n_elyte=64, seed=pref.SEED)
    elif kind == "sparse":
        s = systems.small_random(ne_side=4, n_elyte=64, seed=pref.SEED, cutoff=6.0, lz=200.0, mode="slab")
    elif kind == "manytypes":       # types 16-20: (ntypes + 1)^2 = 441 type pairs, more than the LDS form of the table holds (256)
        s = systems.small_random(ne_side=4, n_elyte=64, seed=pref.SEED)
        s = dataclasses.replace(s, ntypes=20, type=(s.type + 15).astype(np.int32))
    else:
        s = systems.deck(kind, "ffield", etypes=False)
    return dataclasses.replace(s, newton=newton, eletypes=None)


@functools.lru_cache(maxsize=None)
def case(kind, newton, special=False, ghost_images=False, lj=True):
    """a handle after setup_post_neighbor with the pair tables and list set, and the reference at its atoms: formed once per process
    and shared (the entries keep no state between calls)"""
    s = system(kind, newton)
    at, lst, _ = neighbor.build_lists(s, special_frac=0.2 if special else 0.0)
    p = pref.lj_tables(s.ntypes, s.cutoff, with_lj=lj)
    sl, sc = (pref.SPECIAL_LJ, pref.SPECIAL_COUL) if special else (pref.ONES, pref.ONES)
    fx = FixConp(s, ghost_images=ghost_images)
    fx.init_lists(lst, lst)
    fx.setup_post_neighbor(at)
    fx.pair_set_params(p.cutsq, p.cut_coul, p.lj, sl, sc)
    fx.pair_set_list(lst, at.nall)
    return SimpleNamespace(s=s, at=at, lst=lst, p=p, fx=fx, sl=sl, sc=sc, newton=newton, R=pref.for_atoms(at, lst, p, s, newton, sl, sc),
                           tag=f"{kind}, newton {'on' if newton else 'off'}" + (", special" if special else ""))


def _frac(tag, got, want, bound):
    """largest |got - want| / bound over the entries (0 / 0 counts as 0: an entry without terms must be exact)"""
    err = np.abs(np.asarray(got, dtype=np.longdouble) - want)
    bound = np.asarray(bound, dtype=np.longdouble) * np.ones_like(err)
    assert np.all(err[bound == 0] == 0), tag
    fr = float((err[bound > 0] / bound[bound > 0]).max()) if np.any(bound > 0) else 0.0
    print(f"{tag}: {fr:.3g} of the bound")
    return fr


def check(tag, got, R):
    """(f, eng, W, eatom, vatom) of an entry against the reference; None entries are skipped"""
    f, eng, W, ea, va = got
    fr = []
    if f is not None:
        fr.append(_frac(f"{tag}: force", f, R.f, TOL * R.A[:, None]))
    if eng is not None:
        fr.append(_frac(f"{tag}: eng_vdwl, eng_coul", eng, R.eng, TOL * R.E_abs))
    if W is not None:
        fr.append(_frac(f"{tag}: virial", W, R.W, TOL * R.W_abs))
    if ea is not None:
        fr.append(_frac(f"{tag}: eatom", ea, R.eatom, TOL * R.eatom_abs))
    if va is not None:
        fr.append(_frac(f"{tag}: vatom", va, R.vatom, TOL * R.vatom_abs))
    assert max(fr) <= 1.0, (tag, fr)


def test_the_lists_have_the_rows_the_kernel_can_go_wrong_on():
    nn = {k: c.lst.numneigh[c.lst.ilist] for k, c in (("off", case("small", False)), ("on", case("small", True)),
                                                     ("sparse", case("sparse", True)))}
    assert np.any((nn["off"] > 64) & (nn["off"] % 64 != 0))          # several passes of the lane loop, a ragged last one
    assert np.any((nn["on"] > 0) & (nn["on"] < 64))                  # fewer neighbours than lanes
    assert np.any(nn["sparse"] == 0)                                 # a row with none
    for c in (case("small", False), case("small", True), case("sparse", True)):
        assert c.R.rmin >= 0.8, c.R.rmin
    assert case("sparse", True).lst.inum > 4                         # more than one workgroup


@pytest.mark.parametrize("kind,newton", [("small", False), ("small", True), ("sparse", True), ("sparse", False), ("il_onelayer", False)])
def test_matches_the_reference(kind, newton):
    c = case(kind, newton)
    got = c.fx.pair_compute(c.at)
    check(c.tag, got, c.R)
    n = c.at.nlocal
    if not newton:                                                   # ghost entries are not touched
        assert np.all(got[0][n:] == 0) and np.all(got[3][n:] == 0) and np.all(got[4][n:] == 0)
    else:
        assert np.abs(got[0][n:]).max() > 0
    # zero-charge atoms (the electrode atoms before an update) still feel the LJ part
    z = np.nonzero(c.at.q[:n] == 0)[0]
    if kind == "small":
        assert len(z) == 64 and np.abs(got[0][z]).max(axis=1).min() > 0


def test_special_bond_factors():
    c = case("small", False, special=True)
    sb = (c.lst.neigh.astype(np.int64) >> 30) & 3
    assert {1, 2, 3} <= set(np.unique(sb))                           # fc = 0 (bit pattern 1) among them: erfc - 1 is what is left
    check(c.tag, c.fx.pair_compute(c.at), c.R)
    plain = case("small", False).R
    assert abs(c.R.eng[1] - plain.eng[1]) > 1e-6 * plain.E_abs       # (the factors matter at the bound's scale)


@pytest.mark.parametrize("newton", [False, True])
def test_without_the_lj_part(newton):
    c = case("small", newton, lj=False)
    got = c.fx.pair_compute(c.at)
    check(c.tag + ", cut_ljsq NULL", got, c.R)
    assert got[1][0] == 0.0
    z = np.nonzero(c.at.q == 0)[0]
    assert np.all(got[0][z] == 0) and np.all(got[3][z] == 0)         # nothing acts on a zero charge now


def test_forces_are_added_to_what_is_there():
    c = case("small", False)
    n, nall = c.at.nlocal, c.at.nall
    pre = np.random.default_rng(3).normal(size=(nall, 3))
    f = pre.copy()
    c.fx.pair_compute(c.at, f=f, eng=False, virial=False, eatom=False, vatom=False)
    assert np.all(f[n:] == pre[n:])                                  # newton off: ghost rows untouched, bit for bit
    # pre-fill + force: one more rounding, of the sum (|pre| ~ 1, forces up to 1e5)
    _ = _frac("pre-filled f", f - pre, c.R.f, TOL * c.R.A[:, None] + 4e-16 * (np.abs(pre) + np.abs(c.R.f.astype(float))))
    assert _ <= 1.0


def test_each_output_alone_and_all_null():
    c = case("small", True)
    names = ("forces", "eng", "virial", "eatom", "vatom")
    for k, name in enumerate(names):
        on = {m: m == name for m in names}
        got = c.fx.pair_compute(c.at, **on)
        assert [g is not None for g in got] == [m == name for m in names]
        check(f"{name} alone", got, c.R)
    rc = c.fx.lib.conp_pair_compute(c.fx.h, capi.C.byref(c.fx.atoms_view(c.at)), None, None, None, None, None)
    assert rc == 0


def test_eng_and_virial_are_bit_reproducible():
    c = case("small", True)
    a, b = c.fx.pair_compute(c.at), c.fx.pair_compute(c.at)
    assert a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
    only = c.fx.pair_compute(c.at, forces=False, eatom=False, vatom=False)          # (another instantiation, the same sums)
    assert a[1].tobytes() == only[1].tobytes() and a[2].tobytes() == only[2].tobytes()


@pytest.mark.parametrize("newton", [False, True])
def test_ghost_images_upload_path(newton):
    c0, c1 = case("small", newton), case("small", newton, ghost_images=True)
    g0, g1 = c0.fx.pair_compute(c0.at), c1.fx.pair_compute(c1.at)
    check(c1.tag + ", ghost_images", g1, c1.R)
    assert g0[1].tobytes() == g1[1].tobytes() and g0[2].tobytes() == g1[2].tobytes()     # the ghosts rebuilt on the device: same bits
    # moved atoms, ghosts moving with their owners: the entry keeps no cache
    at = dataclasses.replace(c1.at, x=c1.at.x.copy())
    n, prd = at.nlocal, np.asarray(c1.s.prd)
    img = np.round((c1.at.x[n:] - c1.at.x[at.owner[n:]]) / prd)
    assert np.all(c1.at.x[at.owner[n:]] + img * prd == c1.at.x[n:])          # exact images (what the handle verified at post_neighbor)
    at.x[:n] += np.random.default_rng(9).normal(scale=0.01, size=(n, 3))
    at.x[n:] = at.x[at.owner[n:]] + img * prd                                # Comm's arithmetic: x_owner + n * prd
    R = pref.for_atoms(at, c1.lst, c1.p, c1.s, newton)
    assert abs(R.eng.sum() - c1.R.eng.sum()) > 1e-9 * R.E_abs
    g = c1.fx.pair_compute(at)
    g_full = c0.fx.pair_compute(at)
    check(c1.tag + ", moved atoms, ghost_images", g, R)
    check(c0.tag + ", moved atoms", g_full, R)


def test_a_second_set_list_is_what_the_next_call_uses():
    c = case("small", False)
    other = case("sparse", False)
    s = c.s
    fx = FixConp(s)
    fx.init_lists(c.lst, c.lst)
    fx.setup_post_neighbor(c.at)
    fx.pair_set_params(c.p.cutsq, c.p.cut_coul, c.p.lj)
    fx.pair_set_list(c.lst, c.at.nall)
    check("first list", fx.pair_compute(c.at), c.R)
    # the same pairs with the rows visited in another order
    lst2 = dataclasses.replace(c.lst, ilist=np.ascontiguousarray(c.lst.ilist[::-1]))
    fx.pair_set_list(lst2, c.at.nall)
    check("rows reversed", fx.pair_compute(c.at), c.R)
    # another list, another nall (not that of the last post_neighbor: x and q take the plain copy)
    assert other.at.nall != c.at.nall and other.s.ntypes == s.ntypes
    fx.pair_set_list(other.lst, other.at.nall)
    p6 = pref.lj_tables(s.ntypes, s.cutoff)
    R = pref.reference(other.at.x, other.at.q, other.at.type, other.at.nlocal, other.lst, p6, s.g_ewald, systems.QQRD2E, False)
    check("other list, other nall", fx.pair_compute(other.at), R)
    with pytest.raises(ConpError) as e:                              # and the old atoms no longer fit
        fx.pair_compute(c.at)
    assert e.value.code == -1
    fx.close()


def test_types_beyond_the_lds_table():
    c = case("manytypes", True)
    assert (c.s.ntypes + 1) ** 2 > 256 and c.at.type.min() >= 16
    check(c.tag + " (table read from global memory)", c.fx.pair_compute(c.at), c.R)


def test_error_returns():
    c = case("small", False)
    s = c.s
    fx = FixConp(s)
    with pytest.raises(ConpError) as e:                              # before set_params
        fx.pair_compute(c.at)
    assert e.value.code == -2 and "conp_pair_set_params" in str(e.value)
    fx.pair_set_params(c.p.cutsq, c.p.cut_coul, c.p.lj)
    with pytest.raises(ConpError) as e:                              # before set_list
        fx.pair_compute(c.at)
    assert e.value.code == -2 and "conp_pair_set_list" in str(e.value)
    with pytest.raises(ConpError) as e:
        fx.pair_compute_device(1, 1, 1, 0, 0, 0)
    assert e.value.code == -2
    fx.pair_set_list(c.lst, c.at.nall)
    assert fx.lib.conp_pair_compute(fx.h, None, None, None, None, None, None) == -1          # NULL atoms
    short = dataclasses.replace(c.at, nghost=c.at.nghost - 1)
    with pytest.raises(ConpError) as e:                              # nlocal + nghost is not the list's nall
        fx.pair_compute(short)
    assert e.value.code == -1
    with pytest.raises(ConpError) as e:                              # a list that points outside its atoms
        fx.pair_set_list(c.lst, c.at.nlocal)
    assert e.value.code == -1
    nolist = capi.conp_neighlist(inum=c.lst.inum, ilist=capi._iptr(c.lst.ilist), numneigh=capi._iptr(c.lst.numneigh),
                                 first=capi._iptr(c.lst.first), nneigh=int(c.lst.neigh.size))          # neigh stays NULL
    assert fx.lib.conp_pair_set_list(fx.h, capi.C.byref(nolist), c.at.nall) == -1
    with pytest.raises(ConpError) as e:                              # ... and leaves the handle without a list
        fx.pair_compute(c.at)
    assert e.value.code == -2
    wrong = dataclasses.replace(s, ntypes=s.ntypes + 1)
    p = pref.lj_tables(wrong.ntypes, s.cutoff)
    par = capi.conp_pair_params(ntypes=wrong.ntypes, cutsq=capi._dptr(np.ascontiguousarray(p.cutsq)), cut_coul=s.cutoff)
    assert fx.lib.conp_pair_set_params(fx.h, capi.C.byref(par)) == -1                        # ntypes differs from env.ntypes
    # works on a `pppm` handle as well (the entries do not touch the k-space provider)
    fp = FixConp(s, extra_args=["pppm"], pppm_mesh=(12, 12, 48), pppm_order=5)
    fp.pair_set_params(c.p.cutsq, c.p.cut_coul, c.p.lj)
    fp.pair_set_list(c.lst, c.at.nall)
    check("pppm handle", fp.pair_compute(c.at), c.R)
    fp.close()
    fx.close()
