"""-m gpu: conp_ghost_build_device / conp_ghost_fill_device / conp_ghost_fill_int_device / conp_ghost_fold_device / conp_ghost_get /
conp_atoms_wrap_device -- ghost atoms built, updated and folded back on the device against the numpy reference
of tests/ghost_ref.py (itself checked against neighbor.make_ghosts by tests/test_ghost_ref_math.py).

(1) the map and the filled arrays are the reference's and make_ghosts', bit for bit, and two builds give the same bytes;  (2) fill
after a move, with and without d_q, int rows, sentinels behind nall;  (3) the sequential fold at widths 1, 3, 6;  (4) build -> fill ->
list build -> pair forces -> fold on one stream, to the bounds of tests/test_gpu_pair_forces.py;  (5) the remap into the box;
(6) edges and refusals.  tests/test_gpu_ghosts_guard.py repeats (1)-(3) and a case of (4) under guard zones."""
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import ghost_ref as gref
import neigh_ref as nref
import pair_force_ref as pref
from conp_amd import ConpError, FixConp, capi
from test_gpu_pair_forces import _frac, TOL

pytestmark = pytest.mark.gpu

KINDS = ["small", "small127", "sparse", "dilute", "il_onelayer"]
PAD = 64                 # sentinel rows behind nall in every array the entries write
SENT = 7.25


def _dev(a, dtype):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()
    torch.cuda.synchronize()
    return t


def _padded(owned, nall, fill, dtype=np.float64):
    """a device array of nall + PAD rows: the owned rows, ghost rows of `fill`, sentinel rows"""
    owned = np.asarray(owned, dtype=dtype)
    a = np.full((nall + PAD,) + owned.shape[1:], fill, dtype=dtype)
    a[:len(owned)] = owned
    a[nall:] = SENT
    return _dev(a, dtype)


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def ghost_case(kind):
    """the reference of an input, formed once: owned atoms (the leading rows of neigh_ref.inputs' arrays), box, map"""
    inp = nref.inputs(kind, False)
    at, s = inp.at, inp.s
    boxlo, boxhi, periodic, cut = gref.box_of(s)
    n = at.nlocal
    ref = gref.build(at.x[:n], boxlo, boxhi, periodic, cut)
    assert ref.margin >= 1e-9
    return SimpleNamespace(kind=kind, inp=inp, at=at, s=s, n=n, nall=at.nall, box=(boxlo, boxhi, periodic, cut), ref=ref)


def _built(c, fx=None, x=None):
    """(handle, nghost) after one build from the owned coordinates alone"""
    fx = FixConp(c.s) if fx is None else fx
    d_x = _dev(c.at.x[:c.n] if x is None else x, np.float64)
    boxlo, boxhi, periodic, cut = c.box
    return fx, fx.ghost_build_device(d_x.data_ptr(), c.n, boxlo, boxhi, periodic, cut)


@pytest.mark.parametrize("kind", KINDS)
def test_build_equals_the_reference(kind):
    c = ghost_case(kind)
    fx, nghost = _built(c)
    nl, ng, owner, img = fx.ghost_get()
    print(f"{kind}: {c.n} owned, {nghost} ghosts, {c.ref.nshift} shifts")
    assert (nl, ng, nghost) == (c.n, c.ref.nghost, c.ref.nghost) and c.ref.nghost == c.at.nghost
    assert np.array_equal(owner, c.ref.owner) and np.array_equal(img, c.ref.img)
    d_x, d_q = _padded(c.at.x[:c.n], c.nall, np.nan), _padded(c.at.q[:c.n], c.nall, np.nan)
    fx.ghost_fill_device(d_x.data_ptr(), d_q.data_ptr())
    x, q = _host(d_x), _host(d_q)
    assert np.array_equal(x[:c.nall], c.at.x) and np.array_equal(q[:c.nall], c.at.q)          # make_ghosts' arrays, bit for bit
    assert np.all(x[c.nall:] == SENT) and np.all(q[c.nall:] == SENT)
    _, again = _built(c, fx)                                                                    # a second build into the same buffers
    nl2, ng2, owner2, img2 = fx.ghost_get()
    assert again == nghost and owner2.tobytes() == owner.tobytes() and img2.tobytes() == img.tobytes()
    fx.close()


@pytest.mark.parametrize("kind", ["small", "sparse"])
def test_fill_after_a_move(kind):
    c = ghost_case(kind)
    n, nall, r = c.n, c.nall, c.ref
    fx, _ = _built(c)
    rng = np.random.default_rng(21)
    step = rng.uniform(-1.0, 1.0, size=(n, 3))
    step *= (0.3 * rng.uniform(0.0, 1.0, size=(n, 1))) / np.linalg.norm(step, axis=1, keepdims=True)
    x_own = c.at.x[:n] + step
    q_own = c.at.q[:n] + rng.normal(size=n)
    want_x = x_own[r.owner] + r.img * r.prd                          # numpy's x[o] + img * prd: the product first
    for with_q in (False, True):
        d_x, d_q = _padded(x_own, nall, np.nan), _padded(q_own, nall, np.nan)
        fx.ghost_fill_device(d_x.data_ptr(), d_q.data_ptr() if with_q else 0)
        x, q = _host(d_x), _host(d_q)
        assert np.array_equal(x[:n], x_own) and np.array_equal(x[n:nall], want_x) and np.all(x[nall:] == SENT)
        assert np.array_equal(q[:n], q_own) and np.all(q[nall:] == SENT)
        assert np.array_equal(q[n:nall], q_own[r.owner]) if with_q else np.all(np.isnan(q[n:nall]))
    tag = c.at.tag[:n].astype(np.int32)
    for width in (1, 3):
        rows = np.stack([tag * (k + 1) + k for k in range(width)], axis=1)
        d_v = _padded(rows, nall, -1, np.int32)
        fx.ghost_fill_int_device(d_v.data_ptr(), width)
        v = _host(d_v)
        assert np.array_equal(v[:n], rows) and np.array_equal(v[n:nall], rows[r.owner]) and np.all(v[nall:] == int(SENT))
    assert np.array_equal(rows[r.owner][:, 0], c.at.tag[n:])          # ... which is the tag array make_ghosts gives
    fx.close()


@pytest.mark.parametrize("width", [1, 3, 6])
def test_fold(width):
    c = ghost_case("small")
    n, nall, r = c.n, c.nall, c.ref
    fx, _ = _built(c)
    v = np.random.default_rng(30 + width).normal(size=(nall, width))
    want = gref.fold(v, r.owner, n)
    assert np.abs(want[:n] - v[:n]).min() > 0                         # every owner has ghosts here
    out = []
    for _ in range(2):
        d_v = _padded(v, nall, 0.0)
        fx.ghost_fold_device(d_v.data_ptr(), width)
        out.append(_host(d_v))
    got = out[0]
    assert np.array_equal(got[:n], want[:n])                          # the sequential sum, bit for bit
    assert np.array_equal(got[n:nall], v[n:]) and np.all(got[nall:] == SENT)
    assert out[0].tobytes() == out[1].tobytes()
    fx.close()


def _folded_ld(v, owner, n):
    """longdouble rows of all atoms folded onto the owners by the map `owner` [nghost]"""
    return pref.fold(v, np.concatenate([np.arange(n), owner]), n)


@functools.lru_cache(maxsize=None)
def composed(kind, newton):
    """handle after setup_post_neighbor -> ghost build -> fill -> list build -> pair forces (f, eatom, vatom) -> fold (newton on), on one
    stream with one synchronisation at the end.  d_x and d_q start with their ghost rows unset."""
    import torch
    c = ghost_case(kind)
    inp = nref.inputs(kind, newton)
    at, s, n, nall = inp.at, inp.s, c.n, c.nall
    lst = nref.reference(inp)[0]
    p = pref.lj_tables(s.ntypes, s.cutoff)
    fx = FixConp(s)
    fx.init_lists(lst, lst)
    fx.setup_post_neighbor(at)
    fx.pair_set_params(p.cutsq, p.cut_coul, p.lj)
    d_x, d_q = _padded(at.x[:n], nall, np.nan), _padded(at.q[:n], nall, np.nan)
    d_f = torch.zeros((nall, 3), dtype=torch.float64, device="cuda")
    d_e = torch.full((nall,), np.nan, dtype=torch.float64, device="cuda")
    d_v = torch.full((nall, 6), np.nan, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    boxlo, boxhi, periodic, cut = c.box
    nghost = fx.ghost_build_device(d_x.data_ptr(), n, boxlo, boxhi, periodic, cut)
    assert n + nghost == nall
    fx.ghost_fill_device(d_x.data_ptr(), d_q.data_ptr())
    fx.pair_build_list_device(d_x.data_ptr(), n, nall, inp.cutneigh)
    fx.pair_compute_device(d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), 0, d_e.data_ptr(), d_v.data_ptr())
    if newton:
        fx.ghost_fold_device(d_f.data_ptr(), 3)
        fx.ghost_fold_device(d_e.data_ptr(), 1)
        fx.ghost_fold_device(d_v.data_ptr(), 6)
    torch.cuda.synchronize()
    got, _ = fx.pair_get_list()
    R = pref.for_atoms(at, lst, p, s, newton)
    out = SimpleNamespace(c=c, inp=inp, at=at, n=n, nall=nall, lst=lst, got=got, R=R, f=d_f.cpu().numpy(), eatom=d_e.cpu().numpy(),
                          vatom=d_v.cpu().numpy(), x=d_x.cpu().numpy()[:nall])
    fx.close()
    return out


@pytest.mark.parametrize("kind", ["small", "sparse"])
def test_composition_with_the_list_build_and_the_pair_forces(kind):
    from test_gpu_pair_build_list import _same_list
    on, off = composed(kind, True), composed(kind, False)
    n, owner = on.n, on.c.ref.owner
    assert np.array_equal(on.x, on.at.x)
    for r in (on, off):
        _same_list(f"{kind}: the list built from the filled ghosts", r.got, r.nall, r.lst, r.at)
    R = on.R
    assert np.abs(R.f[n:].astype(float)).max() > 0                   # the ghost rows carry forces: there is something to fold
    f_ref, A = _folded_ld(R.f, owner, n), _folded_ld(R.A, owner, n)
    fr = [_frac(f"{kind}: folded owned forces", on.f[:n], f_ref, TOL * A[:, None]),
          _frac(f"{kind}: folded eatom", on.eatom[:n], _folded_ld(R.eatom, owner, n), TOL * _folded_ld(R.eatom_abs, owner, n)),
          _frac(f"{kind}: folded vatom", on.vatom[:n], _folded_ld(R.vatom, owner, n), TOL * _folded_ld(R.vatom_abs, owner, n)),
          # newton off computes every owned atom's force on the owned row itself: the two runs agree within the sum of their bounds
          _frac(f"{kind}: newton on, folded, against newton off", on.f[:n], off.f[:n].astype(np.longdouble),
                TOL * A[:, None] + TOL * off.R.A[:n, None])]
    assert max(fr) <= 1.0, fr
    assert np.all(off.f[n:] == 0)                                    # newton off leaves the ghost rows alone: nothing to fold


@pytest.mark.parametrize("kind", ["small", "sparse"])
def test_wrap(kind):
    c = ghost_case(kind)
    n = c.n
    boxlo, boxhi, periodic, cut = c.box
    prd = boxhi - boxlo
    rng = np.random.default_rng(40)
    x0 = c.at.x[:n] + rng.uniform(-0.9, 0.9, size=(n, 3)) * prd
    x0[3, 0], x0[4, 1], x0[5, 0], x0[6, 1] = boxhi[0], boxhi[1], boxlo[0], boxlo[1]             # exactly on the bounds
    image0 = rng.integers(-3, 4, size=(n, 3)).astype(np.int32)
    want_x, want_image = gref.wrap(x0, boxlo, boxhi, periodic, image0)
    assert np.any(want_image != image0) and (want_x[3, 0], want_x[5, 0]) == (boxlo[0], boxlo[0])
    per = np.array(periodic)
    assert np.all((want_x[:, per] >= boxlo[per]) & (want_x[:, per] < boxhi[per]))
    fx = FixConp(c.s)                                                # (no ghost build is needed)
    d_x, d_i = _padded(x0, n, np.nan), _padded(image0, n, 0, np.int32)
    fx.atoms_wrap_device(d_x.data_ptr(), n, boxlo, boxhi, periodic, d_i.data_ptr())
    x, image = _host(d_x), _host(d_i)
    assert np.array_equal(x[:n], want_x) and np.array_equal(image[:n], want_image)
    assert np.all(x[n:] == SENT) and np.all(image[n:] == int(SENT))
    if kind == "sparse":
        assert not periodic[2] and np.array_equal(x[:n, 2], x0[:, 2]) and np.array_equal(image[:n, 2], image0[:, 2])
        assert np.any(x0[:, 2] < boxlo[2]) and np.any(x0[:, 2] >= boxhi[2])
    d_x2 = _padded(x0, n, np.nan)
    fx.atoms_wrap_device(d_x2.data_ptr(), n, boxlo, boxhi, periodic, 0)                        # without counters
    assert np.array_equal(_host(d_x2), x)
    # wrap, then build: the reference build of the wrapped atoms
    nghost = fx.ghost_build_device(d_x.data_ptr(), n, boxlo, boxhi, periodic, cut)
    r = gref.build(want_x, boxlo, boxhi, periodic, cut)
    _, ng, owner, img = fx.ghost_get()
    assert nghost == ng == r.nghost and np.array_equal(owner, r.owner) and np.array_equal(img, r.img)
    # the three edge atoms of tests/test_ghost_ref_math.py, in their own box
    e = gref.edge_case()
    d_x, d_i = _padded(e.x, 3, np.nan), _padded(np.zeros((3, 3)), 3, 0, np.int32)
    fx.atoms_wrap_device(d_x.data_ptr(), 3, e.boxlo, e.boxhi, e.periodic, d_i.data_ptr())
    assert np.array_equal(_host(d_x)[:3], e.want_x) and np.array_equal(_host(d_i)[:3], e.want_image)
    fx.close()


def test_zero_ghosts():
    c = ghost_case("small")
    boxlo, boxhi, periodic, cut = c.box
    fx = FixConp(c.s)
    d_x = _padded(c.at.x[:c.n], c.n, np.nan)
    d_f = _padded(np.ones((c.n, 3)), c.n, np.nan)
    d_t = _padded(np.ones((c.n, 1)), c.n, 0, np.int32)
    before = _host(d_x).copy(), _host(d_f).copy()
    for nlocal, per, cg in ((0, periodic, cut), (c.n, (False, False, False), cut), (c.n, periodic, 0.0)):
        assert fx.ghost_build_device(d_x.data_ptr(), nlocal, boxlo, boxhi, per, cg) == 0
        nl, ng, owner, img = fx.ghost_get()
        assert (nl, ng, owner.size, img.size) == (nlocal, 0, 0, 0)
        fx.ghost_fill_device(d_x.data_ptr(), 0)                      # no-ops: CONP_OK (anything else raises)
        fx.ghost_fill_int_device(d_t.data_ptr(), 1)
        fx.ghost_fold_device(d_f.data_ptr(), 3)
        assert _host(d_x).tobytes() == before[0].tobytes() and _host(d_f).tobytes() == before[1].tobytes()
    assert fx.ghost_build_device(0, 0, boxlo, boxhi, periodic, cut) == 0                       # NULL d_x without atoms
    fx.ghost_fill_device(0, 0); fx.ghost_fold_device(0, 3)
    # boxhi <= boxlo is no error in a dimension that is not periodic
    assert fx.ghost_build_device(d_x.data_ptr(), c.n, boxlo, [boxhi[0], boxhi[1], boxlo[2]], (True, True, False), 0.0) == 0
    fx.close()


def test_a_coordinate_that_is_not_finite_has_no_images():
    c = ghost_case("small")
    boxlo, boxhi, periodic, cut = c.box
    x = c.at.x[:c.n].copy()
    x[5, 0], x[5, 1] = np.nan, np.inf
    x[70, 2] = -np.inf
    fx, nghost = _built(c, x=x)
    _, ng, owner, img = fx.ghost_get()
    keep = (c.ref.owner != 5) & (c.ref.owner != 70)
    assert np.any(~keep) and nghost == ng == int(keep.sum())
    assert np.array_equal(owner, c.ref.owner[keep]) and np.array_equal(img, c.ref.img[keep])   # the others are unchanged
    fx.close()


def test_refusals():
    c = ghost_case("small")
    boxlo, boxhi, periodic, cut = c.box
    n, prd = c.n, boxhi - boxlo
    d_x = _padded(c.at.x[:n], c.nall, np.nan)
    d_t = _padded(np.ones((n, 1)), c.nall, 0, np.int32)
    fx = FixConp(c.s)

    def state_errors():
        for call in (lambda: fx.ghost_fill_device(d_x.data_ptr(), 0), lambda: fx.ghost_fill_int_device(d_t.data_ptr(), 1),
                     lambda: fx.ghost_fold_device(d_x.data_ptr(), 3), fx.ghost_get):
            with pytest.raises(ConpError) as e:
                call()
            assert e.value.code == -2
    state_errors()                                                   # before any build
    ok = dict(d_x=d_x.data_ptr(), nlocal=n, boxlo=boxlo, boxhi=boxhi, periodic=periodic, cutghost=cut)
    assert 19 ** 3 - 1 > 4096 and 15 ** 3 - 1 <= 4096
    bad = [dict(d_x=0), dict(nlocal=-1), dict(cutghost=-1.0), dict(cutghost=float("nan")), dict(cutghost=float("inf")),
           dict(boxhi=[boxlo[0], boxhi[1], boxhi[2]]), dict(boxhi=[boxhi[0], boxlo[1] - 1.0, boxhi[2]]),
           dict(boxlo=[float("nan"), boxlo[1], boxlo[2]]),
           dict(boxlo=[0.0, 0.0, 0.0], boxhi=[1.0, 1.0, 1.0], periodic=(True, True, True), cutghost=8.5)]     # m = 9: 6858 shifts
    for kw in bad:
        assert fx.ghost_build_device(**ok) == c.ref.nghost
        with pytest.raises(ConpError) as e:
            fx.ghost_build_device(**dict(ok, **kw))
        assert e.value.code == -1 and "conp_ghost_build_device" in str(e.value), kw
        state_errors()                                               # a refused build leaves the handle without ghosts
    vp, ip = capi.C.c_void_p, capi.C.POINTER(capi.C.c_int)
    a = capi.conp_ghost_build_args(nlocal=n, boxlo=(capi.C.c_double * 3)(*boxlo), boxhi=(capi.C.c_double * 3)(*boxhi),
                                   periodic=(capi.C.c_int * 3)(1, 1, 1), cutghost=cut)
    ng = capi.C.c_int()
    assert fx.lib.conp_ghost_build_device(fx.h, vp(d_x.data_ptr()), None, capi.C.byref(ng)) == -1            # NULL a
    assert fx.lib.conp_ghost_build_device(fx.h, vp(d_x.data_ptr()), capi.C.byref(a), ip()) == -1             # NULL nghost
    assert fx.lib.conp_ghost_build_device(fx.h, vp(d_x.data_ptr()), capi.C.byref(a), capi.C.byref(ng)) == 0 and ng.value == c.ref.nghost
    # 15^3 - 1 = 3374 shifts pass the cap (m = 7)
    assert fx.ghost_build_device(d_x.data_ptr(), 2, [0.0] * 3, [1.0] * 3, (True,) * 3, 7.0) <= 2 * 3374
    assert fx.ghost_build_device(**ok) == c.ref.nghost
    for call, code in ((lambda: fx.ghost_fill_device(0, 0), -1), (lambda: fx.ghost_fill_int_device(0, 1), -1),
                       (lambda: fx.ghost_fold_device(0, 3), -1), (lambda: fx.ghost_fill_int_device(d_t.data_ptr(), 0), -1),
                       (lambda: fx.ghost_fill_int_device(d_t.data_ptr(), 9), -1), (lambda: fx.ghost_fold_device(d_x.data_ptr(), 0), -1),
                       (lambda: fx.ghost_fold_device(d_x.data_ptr(), 2), -1), (lambda: fx.ghost_fold_device(d_x.data_ptr(), 4), -1),
                       (lambda: fx.atoms_wrap_device(0, n, boxlo, boxhi, periodic), -1),
                       (lambda: fx.atoms_wrap_device(d_x.data_ptr(), -1, boxlo, boxhi, periodic), -1),
                       (lambda: fx.atoms_wrap_device(d_x.data_ptr(), n, boxhi, boxlo, periodic), -1)):
        with pytest.raises(ConpError) as e:
            call()
        assert e.value.code == code
    fx.ghost_fill_device(d_x.data_ptr(), 0)                          # the argument errors left the map in place
    assert np.array_equal(_host(d_x)[:c.nall], c.at.x)
    fx.close()
    # works on a `pppm` handle as well
    fp = FixConp(c.s, extra_args=["pppm"], pppm_mesh=(12, 12, 48), pppm_order=5)
    assert fp.ghost_build_device(**ok) == c.ref.nghost
    assert np.array_equal(fp.ghost_get()[2], c.ref.owner)
    fp.close()


def test_two_to_the_30_atoms_are_refused():
    """the limit is reachable under the cap of 4096 shifts: a unit box with cutghost 7 has m = 7, 15^3 - 1 = 3374 shifts, and atoms with
    coordinates in [0.25, 0.75) keep every image (lo = -7 <= x + s < 8 = hi), so 318 146 owned atoms have 3374 * 318 146 ghosts:
    nlocal + nghost = 1 073 742 750 >= 2^30.  The count pass and the 64-bit total of the scan see them; nothing is allocated for them.
    (One atom fewer passes the limit and would need 17 GB for the map: not run.)"""
    import torch
    n = 318146
    assert n * 3375 >= 2 ** 30 > (n - 1) * 3375
    c = ghost_case("small")
    fx, nghost = _built(c)
    g = torch.Generator(device="cpu"); g.manual_seed(6)
    d_x = (0.25 + 0.5 * torch.rand((n, 3), dtype=torch.float64, generator=g)).cuda()
    torch.cuda.synchronize()
    with pytest.raises(ConpError) as e:
        fx.ghost_build_device(d_x.data_ptr(), n, [0.0] * 3, [1.0] * 3, (True,) * 3, 7.0)
    assert e.value.code == -4 and "2^30" in str(e.value)
    with pytest.raises(ConpError) as e:                              # ... and the earlier map is gone
        fx.ghost_get()
    assert e.value.code == -2
    # a thousand of these atoms build: every image of every atom, shift by shift
    m = 1000
    assert fx.ghost_build_device(d_x.data_ptr(), m, [0.0] * 3, [1.0] * 3, (True,) * 3, 7.0) == 3374 * m
    _, ng, owner, img = fx.ghost_get()
    assert np.array_equal(owner, np.tile(np.arange(m), 3374)) and np.array_equal(img[::m], gref.shifts([0.0] * 3, [1.0] * 3, (True,) * 3, 7.0)[0])
    fx.close()
