"""-m gpu: conp_pair_build_list_device / conp_pair_list_moved_device / conp_pair_get_list -- the pair style's half list built on the
device against the numpy reference of tests/neigh_ref.py (itself checked by tests/test_neigh_ref_math.py).

(1) the downloaded list, rows sorted, equals the reference exactly, special-bond bits included;  (2) two builds give the same bytes,
and so does the pair entry on them;  (3) forces on the built list to the bounds of tests/test_gpu_pair_forces.py;  (4) the
displacement flag;  (5) update -> build -> pair forces on one stream;  (6) refusals, a NaN coordinate among them."""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import neigh_ref as nref
import pair_force_ref as pref
from conp_amd import ConpError, FixConp, capi, neighbor
from test_gpu_pair_device import _call, _to_device
from test_gpu_pair_forces import _frac, TOL, check, system

pytestmark = pytest.mark.gpu

LIST_CASES = [("small", False), ("small", True), ("small127", False), ("small127", True), ("sparse", False), ("sparse", True),
              ("dilute", False), ("dilute", True), ("il_onelayer", False)]


def _dev(a, dtype):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()
    torch.cuda.synchronize()
    return t


def _factors(special):
    return (pref.SPECIAL_LJ, pref.SPECIAL_COUL) if special else (pref.ONES, pref.ONES)


def _handle(s, special, **kw):
    p = pref.lj_tables(s.ntypes, s.cutoff)
    fx = FixConp(s, **kw)
    fx.pair_set_params(p.cutsq, p.cut_coul, p.lj, *_factors(special))
    return fx, p


def _build(fx, inp, d_x, special, cutneigh=None):
    """one build; with `special` the chain tables of neigh_ref.chain_specials go along as device arrays"""
    at = inp.at
    kw = {}
    if special:
        nsp, sp = nref.chain_specials(at)
        keep = (_dev(at.tag, np.int32), _dev(nsp, np.int32), _dev(sp, np.int32))
        kw = dict(d_tag=keep[0].data_ptr(), d_nspecial=keep[1].data_ptr(), d_special=keep[2].data_ptr(), maxspecial=nref.MAXSPECIAL)
    fx.pair_build_list_device(d_x.data_ptr(), at.nlocal, at.nall, inp.cutneigh if cutneigh is None else cutneigh, prd_half=inp.prd_half, **kw)
    return fx.pair_get_list()


def _reference(inp, special):
    sp = nref.chain_specials(inp.at) if special else None
    return nref.reference(inp, sp, *_factors(special))[0]


def _same_list(tag, got, nall, ref, at):
    n = at.nlocal
    assert nall == at.nall and got.inum == n, tag
    assert np.array_equal(got.ilist, np.arange(n)), tag
    assert np.array_equal(got.numneigh, ref.numneigh), tag                       # ghost rows: zero, as in the reference
    assert np.array_equal(got.first[:n], np.cumsum(got.numneigh[:n]) - got.numneigh[:n]) and np.all(got.first[n:] == 0), tag
    assert got.neigh.size == ref.neigh.size, tag
    assert np.array_equal(nref.sort_rows(n, got.numneigh, got.neigh), ref.neigh), tag


@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("kind,newton", LIST_CASES)
def test_the_list_is_the_reference_list(kind, newton, special):
    inp = nref.inputs(kind, newton)
    fx, _ = _handle(inp.s, special)
    d_x = _dev(inp.at.x, np.float64)
    got, nall = _build(fx, inp, d_x, special)
    ref = _reference(inp, special)
    print(f"{kind}, newton {newton}, special {special}: {got.neigh.size} pairs, rows {got.numneigh[:got.inum].min()}-{got.numneigh[:got.inum].max()}")
    _same_list(f"{kind} {newton} {special}", got, nall, ref, inp.at)
    if special:
        assert np.any(got.neigh < 0) or np.any(got.neigh >> 30)                  # bits were stored
    fx.close()


def test_a_grid_with_capped_cells_and_an_empty_build():
    """ten atoms spread over 1e5 A in every direction: 1e12 cells of cutneigh, far more than the cap -- the cells are enlarged; the atom
    that defines the upper bound lands in the last cell.  And nall = 0, nlocal = 0."""
    s = system("small", False)
    rng = np.random.default_rng(11)
    centres = np.array([[0.0, 0.0, 0.0], [1e5, 1e5, 1e5], [5e4, -3e4, 7e4]])
    x = np.concatenate([c + rng.uniform(-3.0, 3.0, size=(k, 3)) for c, k in zip(centres, (4, 3, 3))])
    x = np.ascontiguousarray(x[rng.permutation(len(x))])
    n = len(x)
    for nlocal in (n, 6):
        at = neighbor.Atoms(nlocal=nlocal, nghost=n - nlocal, x=x, q=np.zeros(n), type=np.ones(n, np.int32), tag=np.arange(1, n + 1, dtype=np.int32),
                            echeck=np.zeros(n, np.int32), owner=np.arange(n, dtype=np.int32))
        inp = SimpleNamespace(s=s, at=at, cutneigh=10.0, newton=False, prd_half=np.zeros(3))
        assert nref.cutoff_margin(inp) >= 1e-9
        fx, _ = _handle(s, False)
        got, nall = _build(fx, inp, _dev(x, np.float64), False)
        ref = _reference(inp, False)
        assert ref.neigh.size >= 6
        _same_list(f"capped grid, nlocal {nlocal}", got, nall, ref, at)
        fx.close()
    fx, _ = _handle(s, False)
    fx.pair_build_list_device(_dev(x, np.float64).data_ptr(), 0, 0, 10.0)
    got, nall = fx.pair_get_list()
    assert (got.inum, nall, got.neigh.size) == (0, 0, 0)
    fx.close()


@functools.lru_cache(maxsize=None)
def forces_case(kind, newton, special):
    """a handle after setup_post_neighbor (its type array is what conp_pair_compute_device reads) with the list BUILT on the device"""
    inp = nref.inputs(kind, newton)
    ref = _reference(inp, special)
    fx, p = _handle(inp.s, special)
    fx.init_lists(ref, ref)
    fx.setup_post_neighbor(inp.at)
    d_x, d_q = _to_device(inp.at)
    got, _ = _build(fx, inp, d_x, special)
    R = pref.for_atoms(inp.at, ref, p, inp.s, newton, *_factors(special))
    return SimpleNamespace(inp=inp, at=inp.at, fx=fx, p=p, ref=ref, lst=got, R=R, d_x=d_x, d_q=d_q, special=special)


@pytest.mark.parametrize("kind,newton,special", [("small", False, False), ("small", True, False), ("sparse", True, False),
                                                 ("small", False, True), ("small", True, True)])
def test_forces_on_the_built_list(kind, newton, special):
    c = forces_case(kind, newton, special)
    got = _call(c.fx, c.d_x, c.d_q, c.at.nall)
    check(f"{kind}, newton {newton}, special {special}: built list", got, c.R)


def test_two_builds_give_the_same_bytes_and_the_same_sums():
    c = forces_case("small", True, True)
    a, _ = _build(c.fx, c.inp, c.d_x, True)
    ev_a = _call(c.fx, c.d_x, c.d_q, c.at.nall, f=False, eatom=False, vatom=False)
    b, _ = _build(c.fx, c.inp, c.d_x, True)
    ev_b = _call(c.fx, c.d_x, c.d_q, c.at.nall, f=False, eatom=False, vatom=False)
    for name in ("ilist", "numneigh", "first", "neigh"):
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), name
    assert ev_a[1].tobytes() == ev_b[1].tobytes() and ev_a[2].tobytes() == ev_b[2].tobytes()
    # a second handle that is GIVEN the downloaded list: the same rows in the same order, the same bits
    fx2, _ = _handle(c.inp.s, True)
    fx2.init_lists(c.ref, c.ref)
    fx2.setup_post_neighbor(c.at)
    fx2.pair_set_list(a, c.at.nall)
    ev_2 = _call(fx2, c.d_x, c.d_q, c.at.nall, f=False, eatom=False, vatom=False)
    assert ev_a[1].tobytes() == ev_2[1].tobytes() and ev_a[2].tobytes() == ev_2[2].tobytes()
    up, nall = fx2.pair_get_list()                                               # get_list of an uploaded list: what went up
    assert nall == c.at.nall and all(getattr(a, k).tobytes() == getattr(up, k).tobytes() for k in ("ilist", "numneigh", "first", "neigh"))
    with pytest.raises(ConpError) as e:                                          # ... and an uploaded list has no build coordinates
        fx2.pair_list_moved_device(c.d_x.data_ptr(), 1.0, c.d_x.data_ptr())
    assert e.value.code == -2
    fx2.close()


def test_moved_flag():
    import torch
    c = forces_case("small", False, False)
    at, skin = c.at, c.inp.s.skin
    assert skin > 0
    flag = torch.full((1,), 7, dtype=torch.int32, device="cuda")

    def moved(x):
        d = _dev(x, np.float64)
        c.fx.pair_list_moved_device(d.data_ptr(), 0.5 * skin, flag.data_ptr())
        torch.cuda.synchronize()
        return int(flag.cpu()[0])
    assert moved(at.x) == 0                                                      # (overwrites the 7)
    u = np.array([2.0, -1.0, 2.0]) / 3.0                                         # a unit vector off the axes
    for i in (0, at.nlocal - 1, 77):
        x = at.x.copy(); x[i] += 0.51 * skin * u
        assert moved(x) == 1, i
        x = at.x.copy(); x[i] += 0.49 * skin * u
        assert moved(x) == 0, i                                                  # overwritten on each call: the 1 is gone
    x = at.x.copy(); x[at.nlocal:] += 5.0 * skin                                 # only ghosts move
    assert moved(x) == 0
    x = at.x.copy(); x[:at.nlocal] += 0.49 * skin * u                            # every owned atom, none far enough
    assert moved(x) == 0
    # a new build takes new coordinates
    x = at.x.copy(); x[3] += 0.51 * skin * u
    assert moved(x) == 1
    moved_inp = SimpleNamespace(at=dataclasses.replace(at, x=x), cutneigh=c.inp.cutneigh, prd_half=c.inp.prd_half)
    _build(c.fx, moved_inp, _dev(x, np.float64), False)
    assert moved(x) == 0 and moved(at.x) == 1
    _build(c.fx, c.inp, c.d_x, False)                                            # (the shared case as it was)


def test_update_build_and_pair_forces_on_one_stream():
    """the charge update writes d_q, the build reads d_x, the pair entry reads both: nothing but the build's own synchronisations
    between them, one at the end"""
    import torch
    s = dataclasses.replace(system("small", False), eletypes=(5,))
    at, alist, blist = neighbor.build_lists(s)
    inp = nref.inputs("small", False)
    assert np.array_equal(inp.at.x, at.x)
    ref = _reference(inp, False)
    fx = FixConp(s)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)
    p = pref.lj_tables(s.ntypes, s.cutoff)
    fx.pair_set_params(p.cutsq, p.cut_coul, p.lj)
    ele = at.echeck != 0
    q_solved = at.q.copy()
    at.q[ele] = 0.0
    nall = at.nall
    d_x, d_q = _to_device(at)
    d_f = torch.zeros((nall, 3), dtype=torch.float64, device="cuda")
    d_pev = torch.zeros(8, dtype=torch.float64, device="cuda")
    flag = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    fx.pre_force_device(d_x.data_ptr(), d_q.data_ptr(), s.potdiff)
    fx.pair_build_list_device(d_x.data_ptr(), at.nlocal, nall, inp.cutneigh)
    fx.pair_list_moved_device(d_x.data_ptr(), 0.5 * s.skin, flag.data_ptr())
    fx.pair_compute_device(d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), d_pev.data_ptr(), 0, 0)
    torch.cuda.synchronize()
    at.q[:] = d_q.cpu().numpy()
    assert np.abs(at.q[ele] - q_solved[ele]).max() <= 1e-8 * np.abs(q_solved[ele]).max()          # the update ran
    assert int(flag.cpu()[0]) == 0
    got, _ = fx.pair_get_list()
    _same_list("one stream", got, nall, ref, at)
    R = pref.for_atoms(at, ref, p, s, False)
    ev = d_pev.cpu().numpy()
    check("update -> build -> pair on one stream", (d_f.cpu().numpy(), ev[:2], ev[2:], None, None), R)
    # the separate result: the same list uploaded to a second handle, the charges the update wrote
    fx2, _ = _handle(system("small", False), False)
    fx2.init_lists(ref, ref)
    fx2.setup_post_neighbor(at)
    fx2.pair_set_list(got, nall)
    sep = _call(fx2, d_x, d_q, nall, eatom=False, vatom=False)
    assert sep[1].tobytes() == ev[:2].tobytes() and sep[2].tobytes() == ev[2:].tobytes()
    fx.close(); fx2.close()


def test_refusals():
    inp = nref.inputs("small", False)
    at, s = inp.at, inp.s
    d_x = _dev(at.x, np.float64)
    tag = _dev(at.tag, np.int32)
    fx = FixConp(s)
    with pytest.raises(ConpError) as e:                                          # before conp_pair_set_params
        fx.pair_build_list_device(d_x.data_ptr(), at.nlocal, at.nall, inp.cutneigh)
    assert e.value.code == -2 and "conp_pair_build_list_device before conp_pair_set_params" in str(e.value)
    fx.close()
    fx, p = _handle(s, True)
    ok = lambda: fx.pair_build_list_device(d_x.data_ptr(), at.nlocal, at.nall, inp.cutneigh)
    bad = [dict(d_x=0), dict(nlocal=at.nall + 1), dict(nlocal=-1), dict(nall=-1, nlocal=0), dict(cutneigh=s.cutoff * (1 - 1e-12)),
           dict(cutneigh=float("nan")), dict(maxspecial=-1, d_tag=tag.data_ptr(), d_nspecial=tag.data_ptr(), d_special=tag.data_ptr()),
           dict(prd_half=(1.0, -1.0, 1.0))]
    bad += [dict(d_tag=tag.data_ptr() if m & 1 else 0, d_nspecial=tag.data_ptr() if m & 2 else 0, d_special=tag.data_ptr() if m & 4 else 0)
            for m in range(1, 7)]                                                # some but not all of the three
    for kw in bad:
        ok()
        a = dict(d_x=d_x.data_ptr(), nlocal=at.nlocal, nall=at.nall, cutneigh=inp.cutneigh)
        a.update(kw)
        with pytest.raises(ConpError) as e:
            fx.pair_build_list_device(**a)
        assert e.value.code == -1, kw
        with pytest.raises(ConpError) as e:                                      # a refused build leaves the handle without a list
            fx.pair_get_list()
        assert e.value.code == -2, kw
    ok()
    assert fx.lib.conp_pair_build_list_device(fx.h, capi.C.c_void_p(d_x.data_ptr()), None) == -1          # NULL a
    fx.pair_build_list_device(d_x.data_ptr(), at.nlocal, at.nall, s.cutoff)      # cutneigh^2 == the largest cutsq: taken
    with pytest.raises(ConpError) as e:
        fx.pair_list_moved_device(0, 1.0, d_x.data_ptr())
    assert e.value.code == -1
    with pytest.raises(ConpError) as e:
        fx.pair_list_moved_device(d_x.data_ptr(), 1.0, 0)
    assert e.value.code == -1
    # works on a `pppm` handle as well
    fp = FixConp(s, extra_args=["pppm"], pppm_mesh=(12, 12, 48), pppm_order=5)
    fp.pair_set_params(p.cutsq, p.cut_coul, p.lj)
    got, nall = _build(fp, inp, d_x, False)
    _same_list("pppm handle", got, nall, _reference(inp, False), at)
    fp.close()
    fx.close()


@pytest.mark.parametrize("value,where", [(float("nan"), 5), (float("inf"), 700), (-float("inf"), 1298), (float("nan"), 1298)])
def test_a_coordinate_that_is_not_finite(value, where):
    """refused before it can become a cell index (and the index arithmetic clamps whatever it is given): owned atom or ghost"""
    c = forces_case("small", False, False)
    inp, at = c.inp, c.at
    fx, _ = _handle(inp.s, False)
    fx.init_lists(c.ref, c.ref)
    fx.setup_post_neighbor(at)
    _build(fx, inp, c.d_x, False)
    x = at.x.copy()
    x[where, where % 3] = value
    with pytest.raises(ConpError) as e:
        fx.pair_build_list_device(_dev(x, np.float64).data_ptr(), at.nlocal, at.nall, inp.cutneigh)
    assert e.value.code == -4
    with pytest.raises(ConpError) as e:
        fx.pair_compute_device(c.d_x.data_ptr(), c.d_q.data_ptr(), 0, 0, 0, 0)
    assert e.value.code == -2
    got, nall = _build(fx, inp, c.d_x, False)                                    # and the next good build is whole
    _same_list("after a refusal", got, nall, c.ref, at)
    fx.close()


def test_two_to_the_31_pairs_are_refused():
    """65 600 atoms inside one cutoff sphere, newton off: 65 600 * 65 599 / 2 = 2 151 647 200 pairs >= 2^31 -- the count pass and the
    64-bit total of the scan see them, nothing is allocated for them"""
    import torch
    s = system("small", False)
    n = 65600
    assert n * (n - 1) // 2 >= 2 ** 31
    fx, _ = _handle(s, False)
    g = torch.Generator(device="cpu"); g.manual_seed(5)
    d_x = torch.rand((n, 3), dtype=torch.float64, generator=g).cuda()
    torch.cuda.synchronize()
    with pytest.raises(ConpError) as e:
        fx.pair_build_list_device(d_x.data_ptr(), n, n, s.cutoff)
    assert e.value.code == -4 and "2^31" in str(e.value)
    with pytest.raises(ConpError) as e:
        fx.pair_get_list()
    assert e.value.code == -2
    # one atom fewer than the limit needs would be 8 GB of list; a quarter of the atoms builds: every pair, rows n-1 .. 0
    m = 4096
    fx.pair_build_list_device(d_x.data_ptr(), m, m, s.cutoff)
    got, _ = fx.pair_get_list()
    assert got.neigh.size == m * (m - 1) // 2 and np.array_equal(got.numneigh, np.arange(m - 1, -1, -1))
    assert np.array_equal(got.neigh[:m - 1], np.arange(1, m))                    # one cell, members ascending: row 0 is 1 .. m-1 in order
    fx.close()
