"""-m gpu: conp_observe_* -- per-group sums of overlapping groups -- against the restatements of
tests/field_ref.py.  The member counts are exact; every other column is entry-wise within 1e-12 of the longdouble reference's
magnitude (n 2^-53 for sums over more than 2^13 atoms); columns 5-8 are exactly 0.0 without d_v and an empty group is a row of 0.0.
x, q, v and the image counters carry 64 sentinel rows behind nlocal (NaN, and a large counter)."""
import ctypes as C
import functools

import numpy as np
import pytest

from conp_amd import ConpError, FixConp, capi, systems
import field_ref as fr
from integrate_ref import BOLTZ, FTM2V, LD, MVV2E

pytestmark = pytest.mark.gpu
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def handle():
    """one handle for all cases: the entries need nothing of the fix but its stream, and no setup call is made on it"""
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
    fx.observe_set_params(c.type, c.mask, c.mass, c.ngroups, c.prd)


def observe(fx, c, with_v=True, image=True):
    """one call on fresh device copies -> d_out [ngroups + 1][10] on the host: the last row is a sentinel row of NaN"""
    d_x, d_q, d_v, d_im = dev(c.x), dev(c.q), dev(c.v), dev(c.image)
    d_out = nans(c.ngroups + 1, fr.OBSERVE_W)
    fx.observe_device(d_x.data_ptr(), d_q.data_ptr(), d_out.data_ptr(), d_v=d_v.data_ptr() if with_v else 0,
                      d_image=d_im.data_ptr() if image else 0)
    out = host(d_out)
    assert host(d_x).tobytes() == c.x.tobytes() and host(d_q).tobytes() == c.q.tobytes() and host(d_v).tobytes() == c.v.tobytes()
    assert np.isnan(out[c.ngroups]).all()
    return out[:c.ngroups]


COLUMNS = (("sum q", slice(1, 2)), ("dipole", slice(2, 5)), ("m v.v", slice(5, 6)), ("m v", slice(6, 9)), ("sum m", slice(9, 10)))


def compare(c, out, with_v=True, image=True, w=None, tag=None):
    n = c.nlocal
    tag = tag or f"{c.tag}, v {with_v}, image {image}"
    w = Worst() if w is None else w
    L, D = fr.observe("ld", c, with_v, image), fr.observe("f64", c, with_v, image)
    assert out.shape == D.shape
    assert out[:, 0].tobytes() == D[:, 0].tobytes(), tag                    # the counts are exact
    for name, cols in COLUMNS:
        w.note(name, fr.frac(f"{tag}: {name}", out[:, cols], L.v[:, cols], fr.tol_of(n) * L.m[:, cols]))
    if not with_v:
        assert not out[:, 5:9].any() and not np.signbit(out[:, 5:9]).any(), tag
    for g in range(c.ngroups):
        if D[g, 0] == 0:
            assert not out[g].any() and not np.signbit(out[g]).any(), (tag, g)
    return w


# ---- the size ladder, per group shape ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", fr.SIZES)
@pytest.mark.parametrize("shape", fr.MASK_SHAPES)
def test_every_block_edge_per_group_shape(shape, n):
    """1 group; 3 nested groups; 16 groups of which one is empty: each with atoms in no group, at 1, B - 1, B, B + 1, 1000 and
    B F + 1 = 65 537 atoms (257 rows of partial sums, one more than a finishing workgroup's threads take in one round)"""
    c = fr.case(f"ladder, {shape}", n, seed=n % 89 + 7 * fr.MASK_SHAPES.index(shape), masks=shape)
    fx = handle()
    set_case(fx, c)
    w = Worst()
    first = None
    for with_v in (True, False):
        for image in (True, False):
            out = observe(fx, c, with_v, image)
            compare(c, out, with_v, image, w)
            first = out if first is None else first
    if shape == "sixteen":
        assert not first[11].any()                                           # the empty group
    # byte-identical from call to call
    assert observe(fx, c).tobytes() == first.tobytes()
    w.line(c.tag)


@pytest.mark.parametrize("n", [fr.B + 1, 1000])
def test_sixteen_groups_and_every_atom_in_all_of_them(n):
    c = fr.full_mask_case(n, seed=3)
    fx = handle()
    set_case(fx, c)
    out = observe(fx, c)
    compare(c, out).line(c.tag)
    assert all(out[g].tobytes() == out[0].tobytes() for g in range(16)) and out[0, 0] == n


def test_equal_masses_sum_to_n_m():
    c = fr.with_(fr.case("equal masses", 1000, seed=11, masks="nested"), mass=np.full(5, 39.948))
    fx = handle()
    set_case(fx, c)
    out = observe(fx, c)
    compare(c, out).line(c.tag)
    L = fr.observe("ld", c)
    for g in range(c.ngroups):
        assert abs(LD(out[g, 9]) - LD(out[g, 0]) * LD(39.948)) <= fr.tol_of(c.nlocal) * L.m[g, 9]


@pytest.mark.parametrize("n", [1000, fr.BIG])
def test_one_group_of_all_atoms_against_the_integrator_s_kinetic_energy(n):
    """column 5 against ke of conp_integrate_temperature_device for the same group: both within the bound of the longdouble
    0.5 mvv2e sum m v.v (not bit for bit: the trees differ)"""
    c = fr.case("all in one group", n, seed=31, masks="one")
    c = fr.with_(c, mask=np.ones(n, dtype=np.int32))
    fx = handle()
    set_case(fx, c)
    out = observe(fx, c)
    compare(c, out).line(c.tag)
    fx.integrate_set_params(c.type, np.zeros(n, dtype=np.int32), c.mass, [0], [3.0 * n - 3.0], [100.0], 2.0, FTM2V, MVV2E, BOLTZ)
    d_v, d_t = dev(c.v), nans(1, 4)
    fx.integrate_temperature_device(d_v.data_ptr(), d_t.data_ptr())
    ke = host(d_t)[0, 1]
    L = fr.observe("ld", c)
    want, mag = LD(0.5) * LD(MVV2E) * L.v[0, 5], LD(0.5) * LD(MVV2E) * L.m[0, 5]
    fa = fr.frac("integrator ke", ke, want, fr.tol_of(n) * mag)
    fb = fr.frac("0.5 mvv2e column 5", 0.5 * MVV2E * out[0, 5], want, fr.tol_of(n) * mag)
    assert fa <= 1.0 and fb <= 1.0
    # the temperature an engine forms from column 5
    t = out[0, 5] * MVV2E / ((3.0 * n - 3.0) * BOLTZ)
    assert t == pytest.approx(host(d_t)[0, 0], rel=1e-12)


def test_the_groups_of_the_il_deck():
    """sol, eleleft, eleright, ele, all on tests/golden/deck_il.npz: eleleft and eleright lie inside ele, sol and ele make up all, and
    the cell is neutral: sum q of `all` is within the bound of 0"""
    c = fr.il_case()
    fx = handle()
    set_case(fx, c)
    out = observe(fx, c)
    compare(c, out).line(c.tag)
    sol, left, right, ele, all_ = out
    assert (sol[0], left[0], right[0], ele[0], all_[0]) == (1280, 416, 416, 2496, 3776)
    L = fr.observe("ld", c)
    assert abs(all_[1]) <= fr.tol_of(c.nlocal) * float(L.m[4, 1])
    assert ele[5] == 0.0 and left[5] == 0.0 and sol[5] > 0.0 and all_[5] == pytest.approx(sol[5], rel=1e-13)
    assert all_[9] == pytest.approx(sol[9] + ele[9], rel=1e-13)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def _raises(code, fn, *a, **k):
    with pytest.raises(ConpError) as e:
        fn(*a, **k)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_refusals_and_special_cases():
    c = fr.case("refusals", 1000, seed=37, masks="nested")
    n = c.nlocal
    fx = FixConp(systems.small_random(ne_side=4, n_elyte=64))
    lib = fx.lib
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    vec = lambda *v: (C.c_double * 3)(*v)
    nan, inf = float("nan"), float("inf")
    mass1 = np.concatenate([[0.0], c.mass])

    def params(**k):
        v = dict(nlocal=n, ntypes=len(c.mass), ngroups=c.ngroups, type=ip(c.type), mask=ip(c.mask), mass=dp(mass1), prd=vec(*c.prd))
        v.update(k)
        return lib.conp_observe_set_params(fx.h, C.byref(capi.conp_observe_params(**v)))
    d_x, d_q, d_v, d_im, d_out = dev(c.x), dev(c.q), dev(c.v), dev(c.image), nans(c.ngroups + 1, fr.OBSERVE_W)
    X, Q, V, IM, O = (t.data_ptr() for t in (d_x, d_q, d_v, d_im, d_out))
    raw = lambda x=X, q=Q, v=V, im=IM, out=O: lib.conp_observe_device(fx.h, x, q, v, im, out)
    untouched = lambda: np.isnan(host(d_out)).all()
    assert raw() == -2 and untouched()                                     # before set_params
    set_case(fx, c)
    want = observe(fx, c)
    compare(c, want).line("before the refusals")

    def still_fine():
        set_case(fx, c)
        assert observe(fx, c).tobytes() == want.tobytes()

    def edited(a, at, val):
        e = a.copy(); e[at] = val
        return e
    bad_types = [edited(c.type, 5, len(c.mass) + 1), edited(c.type, 7, 0), edited(c.type, n - 1, -2)]
    bad_masks = [edited(c.mask, 3, 1 << c.ngroups), edited(c.mask, n - 1, 1 << 20), edited(c.mask, 0, -1)]
    bad_mass = [edited(mass1, 2, 0.0), edited(mass1, 1, -1.0), edited(mass1, 3, nan), edited(mass1, 5, inf)]
    refused = [dict(type=None), dict(mask=None), dict(mass=None), dict(nlocal=-1), dict(ntypes=-1), dict(ngroups=0), dict(ngroups=-1),
               dict(ngroups=17)] + [dict(type=ip(t)) for t in bad_types] + [dict(mask=ip(m)) for m in bad_masks] + \
              [dict(mass=dp(m)) for m in bad_mass] + \
              [dict(prd=vec(-1.0, 0.0, 0.0)), dict(prd=vec(0.0, nan, 0.0)), dict(prd=vec(0.0, 0.0, inf))]
    for k, bad in enumerate(refused):
        assert params(**bad) == -1, (k, bad)
        assert raw() == -2 and untouched(), (k, bad)                      # a refused set_params leaves the handle without groups
        still_fine()
    assert lib.conp_observe_set_params(fx.h, None) == -1
    assert raw() == -2
    still_fine()
    # a mask may hold every bit below ngroups, and 16 groups take bit 15
    assert params(ngroups=16, mask=ip(edited(c.mask, 3, 1 << 15))) == 0
    still_fine()
    # the step entry: NULL pointers change nothing -- the next call gives the unrefused result
    set_case(fx, c)
    for bad in (dict(x=0), dict(q=0), dict(out=0)):
        assert raw(**bad) == -1, bad
        assert untouched()
        assert observe(fx, c).tobytes() == want.tobytes()
    _raises(-1, fx.observe_device, 0, Q, O)
    # nlocal == 0: CONP_OK, d_out zeroed
    e = np.zeros(0, dtype=np.int32)
    fx.observe_set_params(e, e, c.mass, 3)
    assert raw() == 0
    out = host(d_out)
    assert not out[:3].any() and np.isnan(out[3]).all()
    still_fine()
    fx.close()
