"""-m gpu: the conp_efield_* entries -- `fix efield` with a constant field, and the field coupled to the fix scalar of the same update
 -- against the restatements of tests/field_ref.py.  Real units, qe2f = 23.060549.  d_f and d_vatom are bit for
bit the float64 restatement (selected rows v, unselected rows exactly 0.0); x, q, the image counters, the unselected rows of d_f and
the 64 NaN sentinel rows behind nlocal stay bit for bit; d_out[0 .. 9] is entry-wise within 1e-12 of the longdouble reference's
magnitude (n 2^-53 for sums over more than 2^13 atoms) and d_out[10], the count, is exact."""
import ctypes as C
import functools

import numpy as np
import pytest

from conp_amd import ConpError, FixConp, capi, neighbor, systems
import field_ref as fr

pytestmark = pytest.mark.gpu
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def handle():
    """one handle for the uncoupled cases: the entries need nothing of the fix but its stream, and no setup call is made on it"""
    return FixConp(systems.small_random(ne_side=4, n_elyte=64))


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def nans(*shape):
    import torch
    return torch.full(shape, NAN, dtype=torch.float64, device="cuda")


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


class Worst(dict):
    def note(self, key, fr_):
        self[key] = max(self.get(key, 0.0), fr_)

    def line(self, tag):
        print(f"{tag}: largest fraction of the bound: " + ", ".join(f"{k} {v:.3g}" for k, v in self.items()))
        assert max(self.values()) <= 1.0, (tag, dict(self))


def set_case(fx, c):
    fx.efield_set_params(c.sel, c.qe2f, c.prd)


def post_force(fx, c, e, image=True, with_out=True, with_vatom=True, couple=0, couple_scale=0.0, d_xq=None):
    """one call on fresh device copies -> (f, d_out, vatom, x, q, image) on the host, sentinel rows included"""
    n = c.nlocal
    d_x, d_q = (dev(c.x), dev(c.q)) if d_xq is None else d_xq
    d_f, d_im = dev(c.f), dev(c.image)
    d_out = nans(fr.EFIELD_W) if with_out else None
    d_va = nans(n + fr.SENTINELS, 6) if with_vatom else None
    ptr = lambda t: t.data_ptr() if t is not None else 0
    fx.efield_post_force_device(d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), e, d_image=d_im.data_ptr() if image else 0, couple=couple,
                                couple_scale=couple_scale, d_out=ptr(d_out), d_vatom=ptr(d_va))
    return (host(d_f), host(d_out) if with_out else None, host(d_va) if with_vatom else None, host(d_x), host(d_q), host(d_im))


def compare(c, e, got, w=None, tag=None, **opt):
    """the outputs of one call against both restatements"""
    n = c.nlocal
    tag = tag or c.tag
    w = Worst() if w is None else w
    f, out, va, gx, gq, gi = got
    L, D = fr.efield("ld", c, e, **opt), fr.efield("f64", c, e, **opt)
    assert f[:n].tobytes() == D.f.tobytes(), tag
    assert f[n:].tobytes() == c.f[n:].tobytes(), tag
    unsel = c.sel[:n] == 0
    assert f[:n][unsel].tobytes() == c.f[:n][unsel].tobytes(), tag
    assert gx.tobytes() == c.x.tobytes() and gi.tobytes() == c.image.tobytes(), tag
    if opt.get("s") is None:
        assert gq.tobytes() == c.q.tobytes(), tag
    if va is not None:
        assert va[:n].tobytes() == D.vatom.tobytes(), tag
        assert not va[:n][unsel].any() and not np.signbit(va[:n][unsel]).any() and np.isnan(va[n:]).all(), tag
    if out is not None:
        w.note("energy", fr.frac(f"{tag}: energy", out[0], L.out.v[0], fr.tol_of(n) * L.out.m[0]))
        w.note("sum f", fr.frac(f"{tag}: sum f", out[1:4], L.out.v[1:4], fr.tol_of(n) * L.out.m[1:4]))
        w.note("virial", fr.frac(f"{tag}: virial", out[4:10], L.out.v[4:10], fr.tol_of(n) * L.out.m[4:10]))
        assert out[10] == L.nsel, (tag, out[10], L.nsel)
    return w


# ---- the size ladder -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", fr.SIZES)
def test_every_block_edge(n):
    """1, B - 1, B, B + 1, 1000 and B F + 1 = 65 537 atoms: 257 rows of partial sums, one more than the 256 threads of the finishing
    workgroup take in one round"""
    c = fr.case("ladder", n, seed=n % 97)
    e = fr.FIELDS["xyz"]
    fx = handle()
    set_case(fx, c)
    got = post_force(fx, c, e)
    w = compare(c, e, got)
    # d_out and d_vatom each NULL, and both: the same forces, the other output unchanged
    for with_out, with_vatom in ((False, True), (True, False), (False, False)):
        again = post_force(fx, c, e, with_out=with_out, with_vatom=with_vatom)
        assert again[0].tobytes() == got[0].tobytes()
        assert again[1] is None or again[1].tobytes() == got[1].tobytes()
        assert again[2] is None or again[2].tobytes() == got[2].tobytes()
    # byte-identical from call to call
    third = post_force(fx, c, e)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(third, got))
    w.line(c.tag)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("axis", ["x", "y", "z", "xyz"])
def test_a_field_along_each_axis_and_all_three(axis):
    c = fr.case("axes", 1000, seed=5)
    e = fr.FIELDS[axis]
    fx = handle()
    set_case(fx, c)
    got = post_force(fx, c, e)
    compare(c, e, got).line(f"{c.tag}, {axis}")
    if axis != "xyz":
        k = "xyz".index(axis)
        idle = [j for j in range(3) if j != k]
        assert got[0][:c.nlocal][:, idle].tobytes() == c.f[:c.nlocal][:, idle].tobytes()        # q 0.0 added: the same bytes


def test_without_image_counters():
    c = fr.case("axes", 1000, seed=5)
    e = fr.FIELDS["xyz"]
    fx = handle()
    set_case(fx, c)
    got = post_force(fx, c, e, image=False)
    compare(c, e, got, image=False).line(f"{c.tag}, no image")
    with_im = post_force(fx, c, e)
    assert got[0].tobytes() == with_im[0].tobytes() and got[1].tobytes() != with_im[1].tobytes()


@pytest.mark.parametrize("which", ["all selected", "none selected", "zero charges"])
def test_selections_and_zero_charges(which):
    base = fr.case("axes", 1000, seed=5)
    n = base.nlocal
    c = {"all selected": lambda: fr.with_(base, tag=which, sel=np.ones(n, dtype=np.int32)),
         "none selected": lambda: fr.with_(base, tag=which, sel=np.zeros(n, dtype=np.int32)),
         "zero charges": lambda: fr.with_(base, tag=which, q=np.concatenate([np.zeros(n), base.q[n:]]))}[which]()
    e = fr.FIELDS["xyz"]
    fx = handle()
    set_case(fx, c)
    got = post_force(fx, c, e)
    compare(c, e, got).line(which)
    if which == "none selected":
        assert got[0].tobytes() == c.f.tobytes() and not got[1].any() and not got[2][:n].any()
    if which == "zero charges":
        assert got[0].tobytes() == c.f.tobytes() and not got[1][:10].any() and got[1][10] == (c.sel != 0).sum()
    if which == "all selected":
        assert got[1][10] == n


def test_the_dilute_deck():
    """tests/golden/deck_dilute.npz, e = (0, 0, -potdiff / lz) over all atoms: the pinned deck's `fix efield all efield 0 0 $(-1.0/lz)`"""
    c = fr.dilute_case()
    fx = handle()
    set_case(fx, c)
    got = post_force(fx, c, c.e)
    compare(c, c.e, got).line(c.tag)
    n = c.nlocal
    assert got[1][10] == n == 432
    # a neutral cell: the net force is rounding; the energy is -ez times the cell dipole
    L = fr.efield("ld", c, c.e)
    assert abs(got[1][3]) <= fr.TOL * float(L.out.m[3])
    dip = float((c.q[:n] * c.x[:n, 2]).sum())
    assert got[1][0] == pytest.approx(-c.qe2f * c.e[2] * dip, rel=1e-9)


# ---- coupled to the fix scalar ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style", ["conq", "cond"])
def test_the_field_follows_the_fix_scalar_of_the_same_update(style):
    """conp_fix_pre_force_device, then the coupled call on the same stream with no synchronisation between the two; only then
    compute_scalar(): d_f must be bit for bit the float64 rule at that s.  A second update with another prescribed charge gives
    another s and again the matching force."""
    import torch
    s = systems.small_random(ne_side=4, n_elyte=64, mode="ffield")
    at, alist, blist = neighbor.build_lists(s)
    fx = FixConp(s, style=style)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, 0.05)
    n = at.nlocal
    lz = float(s.boxhi[2] - s.boxlo[2])
    base = fr.case("coupled", n, seed=17)
    sel = (at.echeck[:n] == 0).astype(np.int32)
    e = (0.0, 0.0, 0.011)
    seen = []
    for Q in (0.05, 0.083):
        d_x = torch.from_numpy(np.ascontiguousarray(at.x)).cuda()
        d_q = torch.from_numpy(at.q.copy()).cuda()
        c = fr.with_(base, tag=f"{style}, Q {Q}", sel=sel, prd=tuple(float(p) for p in (s.boxhi - s.boxlo)),
                     x=np.ascontiguousarray(np.concatenate([at.x[:n], base.x[n:]])), q=base.q)
        set_case(fx, c)
        d_f, d_im, d_out, d_va = dev(c.f), dev(c.image), nans(fr.EFIELD_W), nans(n + fr.SENTINELS, 6)
        fx.pre_force_device(d_x.data_ptr(), d_q.data_ptr(), Q)
        fx.efield_post_force_device(d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), e, d_image=d_im.data_ptr(), couple=1,
                                    couple_scale=-1.0 / lz, d_out=d_out.data_ptr(), d_vatom=d_va.data_ptr())
        f, out, va, q_new = host(d_f), host(d_out), host(d_va), host(d_q)
        sc = fx.compute_scalar()
        assert np.isfinite(sc) and sc != 0.0
        seen.append(sc)
        c = fr.with_(c, q=np.concatenate([q_new[:n], base.q[n:]]))
        got = (f, out, va, c.x, c.q, c.image)
        compare(c, e, got, couple=1, couple_scale=-1.0 / lz, s=sc).line(c.tag)
        # and against the route it replaces: the scalar on the host, the field formed there, an uncoupled call
        plain = post_force(fx, c, (0.0, 0.0, e[2] + (-1.0 / lz) * sc))
        assert plain[0].tobytes() == f.tobytes()
    assert seen[0] != seen[1]
    fx.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def _raises(code, fn, *a, **k):
    with pytest.raises(ConpError) as e:
        fn(*a, **k)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_refusals_and_special_cases():
    c = fr.case("refusals", 1000, seed=23)
    n = c.nlocal
    e = fr.FIELDS["xyz"]
    fx = FixConp(systems.small_random(ne_side=4, n_elyte=64))          # a conp handle, never set up
    lib = fx.lib
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    vec = lambda *v: (C.c_double * 3)(*v)
    nan, inf = float("nan"), float("inf")

    def params(**k):
        v = dict(nlocal=n, sel=ip(c.sel), qe2f=c.qe2f, prd=vec(*c.prd))
        v.update(k)
        return lib.conp_efield_set_params(fx.h, C.byref(capi.conp_efield_params(**v)))
    d_x, d_q, d_f, d_im, d_out, d_va = dev(c.x), dev(c.q), dev(c.f), dev(c.image), nans(fr.EFIELD_W), nans(n + fr.SENTINELS, 6)
    X, Q, Fp, IM, O, VA = (t.data_ptr() for t in (d_x, d_q, d_f, d_im, d_out, d_va))
    ev = vec(*e)

    def raw(x=X, q=Q, im=IM, f=Fp, e_=ev, couple=0, scale=0.0, out=O, va=VA):
        return lib.conp_efield_post_force_device(fx.h, x, q, im, f, e_, couple, scale, out, va)

    def untouched():
        assert host(d_f).tobytes() == c.f.tobytes() and np.isnan(host(d_out)).all() and np.isnan(host(d_va)).all()
    # before set_params
    assert raw() == -2
    untouched()
    set_case(fx, c)
    want = post_force(fx, c, e)
    compare(c, e, want).line("before the refusals")

    def still_fine():
        set_case(fx, c)
        assert all(p.tobytes() == q.tobytes() for p, q in zip(post_force(fx, c, e), want))
    refused = [dict(sel=None), dict(nlocal=-1), dict(qe2f=nan), dict(qe2f=inf), dict(qe2f=-inf), dict(prd=vec(-1.0, 0.0, 0.0)),
               dict(prd=vec(0.0, nan, 0.0)), dict(prd=vec(0.0, 0.0, inf))]
    for bad in refused:
        assert params(**bad) == -1, bad
        assert raw() == -2, bad                      # a refused set_params leaves the handle without a field
        untouched()
        still_fine()
    assert lib.conp_efield_set_params(fx.h, None) == -1
    assert raw() == -2
    still_fine()
    # the step entry: every refusal changes nothing, and the next call gives the unrefused result
    set_case(fx, c)
    calls = [dict(x=0), dict(q=0), dict(f=0), dict(e_=None), dict(e_=vec(nan, 0.0, 0.0)), dict(e_=vec(0.0, inf, 0.0)),
             dict(e_=vec(0.0, 0.0, -inf)), dict(scale=nan), dict(scale=inf), dict(couple=2), dict(couple=-1),
             dict(couple=1, scale=-0.01)]           # coupled on a conp handle
    for bad in calls:
        assert raw(**bad) == -1, bad
        untouched()
        assert all(p.tobytes() == q.tobytes() for p, q in zip(post_force(fx, c, e), want)), bad
    _raises(-1, fx.efield_post_force_device, X, Q, Fp, e, couple=1, couple_scale=-0.01)
    # nlocal == 0: CONP_OK, d_out zeroed, nothing else touched
    fx.efield_set_params(np.zeros(0, dtype=np.int32), c.qe2f, c.prd)
    assert raw() == 0
    assert host(d_f).tobytes() == c.f.tobytes() and not host(d_out).any() and np.isnan(host(d_va)).all()
    still_fine()
    fx.close()


@pytest.mark.parametrize("style", ["conq", "cond"])
def test_a_coupled_call_before_the_first_update_is_out_of_order(style):
    s = systems.small_random(ne_side=4, n_elyte=64, mode="ffield")
    fx = FixConp(s, style=style)
    c = fr.case("early", 257, seed=29)
    set_case(fx, c)
    d_x, d_q, d_f = dev(c.x), dev(c.q), dev(c.f)
    _raises(-2, fx.efield_post_force_device, d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), (0.0, 0.0, 0.01), couple=1, couple_scale=-0.02)
    assert host(d_f).tobytes() == c.f.tobytes()
    # uncoupled, the same handle serves
    got = post_force(fx, c, fr.FIELDS["z"])
    compare(c, fr.FIELDS["z"], got).line(f"{style}, uncoupled before setup")
    fx.close()
