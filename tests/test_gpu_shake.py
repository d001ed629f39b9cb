"""-m gpu: the conp_shake_* entries -- SHAKE bond and angle constraints -- against the restatements of
tests/shake_ref.py.  Flags 1 and 3 use nothing but + - * / and comparisons: d_f, d_vatom (and x after `correct`) are bit for bit the
float64 restatement and the largest niter is equal; flag 2 (a square root) and every sum over clusters are entry-wise within 1e-12
of the longdouble reference's first-order magnitude (n 2^-53 for sums of more than 2^13 clusters).  x, v and f carry 64 sentinel
rows behind nlocal and a tenth of the atoms are in no cluster: all of these stay bit for bit.  Every longdouble run asserts the
input condition (no |l_new - l| within 1e-9 tolerance of the tolerance), so that both number types iterate equally often."""
import ctypes as C
import functools

import numpy as np
import pytest

from conp_amd import ConpError, FixConp, capi, systems
import bonded_ref as br  # noqa: F401  (shake_ref.reference_steps drives it)
import integrate_ref as ir
import shake_ref as sr

pytestmark = pytest.mark.gpu
LD = np.longdouble
NAN = float("nan")


@functools.lru_cache(maxsize=None)
def handle():
    """one handle for most cases: the entries need nothing of the fix but its stream, and no setup call is made on it"""
    return FixConp(systems.small_random(ne_side=4, n_elyte=64))


def set_case(fx, c):
    fx.shake_set_params(c.type, c.mass, c.bond_d, c.angle_d, c.cluster, c.tolerance, c.max_iter, c.dt, c.ftm2v, c.prd)


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


def idle_rows(c):
    return np.concatenate([~c.member, np.full(sr.SENTINELS, True)])


def bitwise_rows(c):
    """the atoms of flag-1 and flag-3 clusters: their rows are bit for bit the float64 restatement"""
    m = np.zeros(c.nlocal, dtype=bool)
    for row in c.cluster:
        if row[0] != 2:
            m[row[1:4]] = True
    return m


class Worst(dict):
    def note(self, key, fr):
        self[key] = max(self.get(key, 0.0), fr)

    def line(self, tag):
        print(f"{tag}: largest fraction of the bound: " + ", ".join(f"{k} {v:.3g}" for k, v in self.items()))
        assert max(self.values()) <= 1.0, (tag, dict(self))


def post_force(fx, c, x=None, setup=False, with_out=True, with_vatom=True):
    """one call on fresh device copies -> (f, d_out, vatom, x, v) on the host; vatom has the sentinel rows too"""
    n = c.nlocal
    d_x, d_v, d_f = dev(c.x if x is None else x), dev(c.v), dev(c.f)
    d_out = nans(9) if with_out else None
    d_va = nans(n + sr.SENTINELS, 6) if with_vatom and not setup else None
    ptr = lambda t: t.data_ptr() if t is not None else 0
    if setup:
        fx.shake_setup_device(d_x.data_ptr(), d_v.data_ptr(), d_f.data_ptr(), ptr(d_out))
    else:
        fx.shake_post_force_device(d_x.data_ptr(), d_v.data_ptr(), d_f.data_ptr(), ptr(d_out), ptr(d_va))
    return (host(d_f), host(d_out) if with_out else None, host(d_va) if d_va is not None else None, host(d_x), host(d_v))


def compare(c, got, x=None, half=False, w=None, tag=None):
    """the outputs of post_force / setup against both restatements -> the longdouble result"""
    n = c.nlocal
    tag = tag or c.tag
    w = Worst() if w is None else w
    f, out, va, gx, gv = got
    x0 = c.x if x is None else x
    L, F = sr.Rule("ld", c), sr.Rule("f64", c)
    a, b = L.solve(x0[:n], c.v[:n], c.f[:n], half=half), F.solve(x0[:n], c.v[:n], c.f[:n], half=half)
    assert sr.clear_of_the_tolerance(L, c.tolerance) > 1e-9, tag
    bw, idle = bitwise_rows(c), idle_rows(c)
    assert f[:n][bw].tobytes() == b.out[bw].tobytes(), tag
    w.note("f", sr.frac(f"{tag}: f", f[:n], a.out.v, sr.TOL * a.out.m))
    assert f[idle].tobytes() == c.f[idle].tobytes() and gx.tobytes() == x0.tobytes() and gv.tobytes() == c.v.tobytes(), tag
    if va is not None:
        assert va[:n][bw].tobytes() == b.vatom[bw].tobytes(), tag
        w.note("vatom", sr.frac(f"{tag}: vatom", va[:n], a.vatom.v, sr.TOL * a.vatom.m))
        assert not va[:n][~c.member].any() and not np.signbit(va[:n][~c.member]).any() and np.isnan(va[n:]).all(), tag
    if out is not None:
        val, mag = L.d_out(a)
        w.note("virial", sr.frac(f"{tag}: virial", out[:6], val[:6], sr.tol_of(c.ncluster) * mag[:6]))
        assert tuple(out[6:]) == tuple(float(q) for q in val[6:]) == tuple(F.d_out(b)[0][6:]), (tag, out[6:], val[6:])
    return a, w


# ---- the size ladder -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sr.SIZES)
@pytest.mark.parametrize("flag", [1, 3, 2])
def test_every_block_edge_per_flag(flag, n):
    """1, 63, 64, 65 = SHAKE_BLOCK - 1, SHAKE_BLOCK, SHAKE_BLOCK + 1, 1000, and SHAKE_BLOCK * SHAKE_FINISH + 1 = 16385 clusters: 257
    rows of partial sums, one more than the 256 threads of the finishing workgroup take in one round"""
    c = sr.ladder_case(flag, n)
    fx = handle()
    set_case(fx, c)
    got = post_force(fx, c)
    a, w = compare(c, got)
    assert got[1][6] == 0 and got[1][7] == 0 and (got[1][8] == 0) == (flag == 2)
    # without d_out and d_vatom: one launch, the same forces
    again = post_force(fx, c, with_out=False, with_vatom=False)
    assert again[0].tobytes() == got[0].tobytes()
    # and byte-identical from call to call
    third = post_force(fx, c)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(third, got))
    w.line(c.tag)


def test_mixed_flags_interleaved_in_one_call():
    c = sr.mixed_case()
    fx = handle()
    set_case(fx, c)
    got = post_force(fx, c)
    _, w = compare(c, got)
    w.line(c.tag)


@pytest.mark.parametrize("where", ["x", "y", "z", "xyz"])
def test_clusters_across_the_box(where):
    """members on both sides of a face (of three faces at a corner) with prd > 0; the same input with the members unwrapped and
    prd = 0 gives the same forces to the bound"""
    c = sr.straddle_case(where)
    u = sr.unwrapped(c)
    fx = handle()
    set_case(fx, c)
    got = post_force(fx, c)
    a, w = compare(c, got)
    set_case(fx, u)
    flat = post_force(fx, u)
    b, w = compare(u, flat, w=w)
    n = c.nlocal
    w.note("wrapped against unwrapped", sr.frac(f"{c.tag}: f against the unwrapped input", got[0][:n], flat[0][:n], sr.TOL * (a.out.m + b.out.m)))
    w.note("wrapped against unwrapped", sr.frac(f"{c.tag}: virial against the unwrapped input", got[1][:6], flat[1][:6],
                                                  sr.TOL * (a_mag(c, a) + a_mag(u, b))))
    w.line(c.tag)


def a_mag(c, res):
    return sr.Rule("ld", c).d_out(res)[1][:6]


# ---- the real thing ----------------------------------------------------------------------------------------------------------------------
def test_the_cations_of_the_il_deck():
    """correct -> check -> post_force on the 320 three-atom clusters of the deck file, whose wrapped coordinates split molecules
    across the box in x and y"""
    c = sr.deck_case()
    n = c.nlocal
    fx = handle()
    set_case(fx, c)
    L, F = sr.Rule("ld", c), sr.Rule("f64", c)
    before = L.check(c.x[:n])
    d_x, d_two = dev(c.x), nans(2)
    fx.shake_check_device(d_x.data_ptr(), d_two.data_ptr())
    two = host(d_two)
    assert abs(two[0] - before[0]) <= 1e-12 and abs(two[1] - before[1]) <= 1e-12 and two[0] > 0.01
    fx.shake_correct_device(d_x.data_ptr())
    fx.shake_check_device(d_x.data_ptr(), d_two.data_ptr())
    x1, two = host(d_x), host(d_two)
    xl, xf = L.solve(c.x[:n], None, None, correct=True), F.solve(c.x[:n], None, None, correct=True)
    assert sr.clear_of_the_tolerance(L, c.tolerance) > 1e-9
    assert x1[:n].tobytes() == xf.out.tobytes() and x1[idle_rows(c)].tobytes() == c.x[idle_rows(c)].tobytes()
    left = L.check(xl.out)
    w = Worst()
    w.note("x", sr.frac("deck, correct: x", x1[:n], xl.out.v, sr.TOL * xl.out.m))
    print(f"deck: deviation {float(before[0]):.3g}, {float(before[1]):.3g} -> {two[0]:.3g}, {two[1]:.3g} (reference {float(left[0]):.3g}, {float(left[1]):.3g})")
    slack = 6 * sr.TOL * float(xl.out.m.max()) / sr.BOND_D.min()
    assert two[0] <= left[0] + slack and two[1] <= left[1] + slack and two[0] < 1e-5
    got = post_force(fx, c, x=x1)
    compare(c, got, x=x1, w=w)
    w.line(c.tag)


# ---- setup, correct -----------------------------------------------------------------------------------------------------------------------
def test_setup_is_post_force_at_half_dtfsq_and_correct_moves_only_cluster_atoms():
    c = sr.mixed_case()
    n = c.nlocal
    fx = handle()
    set_case(fx, c)
    full = post_force(fx, c)
    half = post_force(fx, c, setup=True)
    _, w = compare(c, half, half=True, tag=c.tag + ", setup")
    assert np.all((half[0] - c.f)[:n][c.member] != (full[0] - c.f)[:n][c.member])
    d_x = dev(c.x)
    fx.shake_correct_device(d_x.data_ptr())
    x1 = host(d_x)
    L, F = sr.Rule("ld", c), sr.Rule("f64", c)
    xl, xf = L.solve(c.x[:n], None, None, correct=True), F.solve(c.x[:n], None, None, correct=True)
    assert sr.clear_of_the_tolerance(L, c.tolerance) > 1e-9
    bw = bitwise_rows(c)
    assert x1[:n][bw].tobytes() == xf.out[bw].tobytes() and x1[idle_rows(c)].tobytes() == c.x[idle_rows(c)].tobytes()
    assert np.all(x1[:n][c.member] != c.x[:n][c.member])
    w.note("x", sr.frac("correct: x", x1[:n], xl.out.v, sr.TOL * xl.out.m))
    d_two = nans(2)
    fx.shake_check_device(d_x.data_ptr(), d_two.data_ptr())
    left = L.check(xl.out)
    slack = 6 * sr.TOL * float(xl.out.m.max()) / sr.BOND_D.min()
    two = host(d_two)
    assert two[0] <= left[0] + slack and two[1] <= left[1] + slack
    w.line(c.tag + ", setup and correct")


# ---- the loop's exits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("max_iter", [1, 2])
def test_a_loop_cut_short_is_counted_and_its_forces_are_the_restatements(max_iter):
    c = sr.strong_case(max_iter)
    fx = handle()
    set_case(fx, c)
    got = post_force(fx, c)
    _, w = compare(c, got)
    assert got[1][6] == c.ncluster and got[1][7] == 0 and got[1][8] == max_iter
    w.line(c.tag)


def test_zero_and_negative_determinants_are_counted():
    """a flag-3 and a flag-1 cluster with determ == 0 add nothing; a flag-2 cluster with a negative discriminant takes determ = 0"""
    c = sr.special_case()
    n = c.nlocal
    fx = handle()
    set_case(fx, c)
    got = post_force(fx, c)
    _, w = compare(c, got)
    assert got[1][6] == 0 and got[1][7] == 3
    for row in c.cluster[c.first_special:c.first_special + 2]:
        assert got[0][row[1:4]].tobytes() == c.f[row[1:4]].tobytes() and not got[2][row[1:4]].any()
    F = sr.Rule("f64", c)
    b = F.solve(c.x[:n], c.v[:n], c.f[:n])
    assert got[0][:n].tobytes() == b.out.tobytes()                    # sqrt(0) is exact: the flag-2 cluster too
    d_x = dev(c.x)
    fx.shake_correct_device(d_x.data_ptr())
    x1 = host(d_x)
    # (for `correct` v counts as 0, s = r and no determinant vanishes: the constructed clusters move like the others)
    xf = F.solve(c.x[:n], None, None, correct=True).out
    bw = bitwise_rows(c)
    assert x1[:n][bw].tobytes() == xf[bw].tobytes() and x1[idle_rows(c)].tobytes() == c.x[idle_rows(c)].tobytes()
    w.line(c.tag)


# ---- device steps ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("style", [0, 1], ids=["nve", "nvt"])
def test_three_device_steps_on_one_stream(style):
    """correct -> bonded -> shake setup -> integrate setup, then three times integrate_initial -> check -> zero d_f ->
    bonded_compute_device -> shake_post_force_device -> integrate_final, with ONE synchronisation behind the last, against the
    longdouble integrator driven by bonded_ref and shake_ref; repeated byte for byte"""
    import torch
    c = sr.step_case(style)
    n, g = c.nlocal, c.integ
    ref = sr.reference_steps(c)
    assert ref.near > 1e-9
    fx = FixConp(systems.small_random(ne_side=4, n_elyte=64))
    fx.set_stream(torch.cuda.current_stream().cuda_stream)               # torch's zero_() and the entries on ONE stream
    set_case(fx, c)
    fx.integrate_set_params(g.type, g.group, g.mass, g.style, g.dof, g.t_period, g.dt, g.ftm2v, g.mvv2e, g.boltz)
    fx.bonded_set_params(c.p.bond_k, c.p.bond_r0, c.p.angle_k, c.p.angle_theta0, newton_bond=True)
    fx.bonded_set_lists(n, n, None, c.angles, c.prd)

    def run():
        d_x, d_v, d_f = dev(c.x[:n]), dev(c.v[:n]), dev(np.zeros((n, 3)))
        d_out, d_sh, d_chk = nans(1, 4), nans(9), [nans(2) for _ in range(3)]
        X, V, Fp = d_x.data_ptr(), d_v.data_ptr(), d_f.data_ptr()
        torch.cuda.synchronize()
        fx.shake_correct_device(X)
        fx.bonded_compute_device(X, Fp, 0, 0, 0)
        fx.shake_setup_device(X, V, Fp, 0)
        fx.integrate_setup_device(V, g.t_target)
        for k in range(3):
            fx.integrate_initial_device(X, V, Fp, g.t_target)
            fx.shake_check_device(X, d_chk[k].data_ptr())
            d_f.zero_()
            fx.bonded_compute_device(X, Fp, 0, 0, 0)
            fx.shake_post_force_device(X, V, Fp, d_sh.data_ptr(), 0)
            fx.integrate_final_device(V, Fp, d_out.data_ptr())
        torch.cuda.synchronize()
        return [t.cpu().numpy() for t in [d_x, d_v, d_f, d_out, d_sh] + d_chk]
    a = run()
    w = Worst()
    # (the reference's bonded forces are those of its x rounded to float64; the device's x differs by rounding, which an angle constant
    #  of 55 kcal/mol/rad^2 turns into far less than the bound)
    w.note("x", sr.frac("3 steps: x", a[0], ref.x.v, sr.TOL * ref.x.m))
    w.note("v", sr.frac("3 steps: v", a[1], ref.v.v, sr.TOL * ref.v.m))
    w.note("f", sr.frac("3 steps: f", a[2], ref.f.v, sr.TOL * ref.f.m))
    val, mag = ir.out_arrays(ref.rows)
    w.note("integrate d_out", sr.frac("3 steps: integrate d_out", a[3], val, sr.TOL * mag))
    w.note("virial", sr.frac("3 steps: virial", a[4][:6], ref.shake[0][:6], sr.TOL * ref.shake[1][:6]))
    assert tuple(a[4][6:]) == tuple(float(q) for q in ref.shake[0][6:])
    slack = 6 * sr.TOL * float(ref.x.m.max()) / sr.BOND_D.min()
    for k in range(3):
        print(f"step {k}: deviation after initial {a[5 + k][0]:.3g}, {a[5 + k][1]:.3g} (reference {float(ref.check[k][0]):.3g}, {float(ref.check[k][1]):.3g})")
        assert a[5 + k][0] <= ref.check[k][0] + slack and a[5 + k][1] <= ref.check[k][1] + slack
        assert a[5 + k][0] < 0.1 * c.tolerance
    moved = np.abs(a[0] - c.x[:n])
    assert np.median(moved) > 1e6 * float(np.median(sr.TOL * ref.x.m))                          # the atoms went somewhere
    w.line(c.tag)
    set_case(fx, c)
    fx.integrate_set_params(g.type, g.group, g.mass, g.style, g.dof, g.t_period, g.dt, g.ftm2v, g.mvv2e, g.boltz)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(run(), a))
    fx.close()


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------------
def _raises(code, fn, *a, **k):
    with pytest.raises(ConpError) as e:
        fn(*a, **k)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_refusals_and_special_cases():
    c = sr.mixed_case()
    n = c.nlocal
    fx = FixConp(systems.small_random(ne_side=4, n_elyte=64))
    lib = fx.lib
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    lead = lambda a: np.concatenate([[0.0], a])
    mass1, bd1, ad1 = lead(c.mass), lead(c.bond_d), lead(c.angle_d)
    cl = np.ascontiguousarray(c.cluster, dtype=np.int32)

    def params(**k):
        v = dict(nlocal=n, ntypes=len(c.mass), type=ip(c.type), mass=dp(mass1), nbondtypes=2, nangletypes=1, bond_distance=dp(bd1),
                 angle_distance=dp(ad1), ncluster=c.ncluster, cluster=ip(cl), tolerance=c.tolerance, max_iter=c.max_iter, dt=c.dt,
                 ftm2v=c.ftm2v, prd=(C.c_double * 3)(*c.prd))
        v.update(k)
        return lib.conp_shake_set_params(fx.h, C.byref(capi.conp_shake_params(**v)))
    d_x, d_v, d_f, d_out, d_va, d_two = dev(c.x), dev(c.v), dev(c.f), nans(9), nans(n + sr.SENTINELS, 6), nans(2)
    X, V, Fp, O, VA, T = (t.data_ptr() for t in (d_x, d_v, d_f, d_out, d_va, d_two))
    # before set_params: every other entry is out of order
    for call in (lambda: lib.conp_shake_correct_device(fx.h, X), lambda: lib.conp_shake_setup_device(fx.h, X, V, Fp, O),
                 lambda: lib.conp_shake_post_force_device(fx.h, X, V, Fp, O, VA), lambda: lib.conp_shake_check_device(fx.h, X, T)):
        assert call() == -2
    set_case(fx, c)
    want = post_force(fx, c)
    compare(c, want)[1].line("before the refusals")

    def still_fine():
        set_case(fx, c)
        assert all(p.tobytes() == q.tobytes() for p, q in zip(post_force(fx, c), want))
    nan, inf = float("nan"), float("inf")
    first = lambda flag: int(np.nonzero(cl[:, 0] == flag)[0][0])

    def edit(row, col, val):
        e = cl.copy(); e[row, col] = val
        return e
    k1, k2, k3 = first(1), first(2), first(3)
    other = cl[k1 + 1] if k1 + 1 < len(cl) else cl[0]
    t_hi, t_0 = c.type.copy(), c.type.copy()
    t_hi[5] = len(c.mass) + 1; t_0[7] = 0
    arrays = dict(m_0=(mass1, 2, 0.0), m_neg=(mass1, 1, -1.0), m_nan=(mass1, 3, nan), m_inf=(mass1, 1, inf), b_0=(bd1, 1, 0.0),
                  b_nan=(bd1, 2, nan), b_inf=(bd1, 2, inf), a_0=(ad1, 1, 0.0), a_neg=(ad1, 1, -5.0))
    bad_arr = {}
    for name, (src, at, val) in arrays.items():
        e = src.copy(); e[at] = val
        bad_arr[name] = e
    clusters = [edit(k1, 0, 4), edit(k2, 0, 0), edit(k3, 0, 5), edit(k1, 1, -1), edit(k1, 2, n), edit(k3, 3, n + 5), edit(k2, 2, -3),
                edit(k1, 2, cl[k1, 1]), edit(k3, 3, cl[k3, 2]), edit(k2, 2, cl[k2, 1]), edit(k1, 3, other[1]), edit(k2, 1, cl[k3, 2]),
                edit(k1, 4, 0), edit(k1, 5, 3), edit(k2, 4, 3), edit(k3, 5, 0), edit(k1, 6, 0), edit(k1, 6, 2)]
    refused = [dict(type=None), dict(mass=None), dict(bond_distance=None), dict(angle_distance=None), dict(cluster=None),
               dict(nlocal=-1), dict(ntypes=-1), dict(nbondtypes=-1), dict(nangletypes=-1), dict(ncluster=-1),
               dict(type=ip(t_hi)), dict(type=ip(t_0))] + [dict(cluster=ip(e)) for e in clusters] + \
              [dict(mass=dp(bad_arr[k])) for k in ("m_0", "m_neg", "m_nan", "m_inf")] + \
              [dict(bond_distance=dp(bad_arr[k])) for k in ("b_0", "b_nan", "b_inf")] + \
              [dict(angle_distance=dp(bad_arr[k])) for k in ("a_0", "a_neg")] + \
              [dict(dt=0.0), dict(dt=-1.0), dict(dt=nan), dict(ftm2v=0.0), dict(ftm2v=inf), dict(tolerance=0.0), dict(tolerance=-1e-4),
               dict(tolerance=nan), dict(tolerance=inf), dict(max_iter=0), dict(max_iter=-3),
               dict(prd=(C.c_double * 3)(-1.0, 0.0, 0.0)), dict(prd=(C.c_double * 3)(0.0, nan, 0.0)), dict(prd=(C.c_double * 3)(0.0, 0.0, inf))]
    for k, bad in enumerate(refused):
        assert params(**bad) == -1, (k, bad)
        # a refused set_params leaves the handle without constraints
        assert lib.conp_shake_post_force_device(fx.h, X, V, Fp, O, VA) == -2 and lib.conp_shake_check_device(fx.h, X, T) == -2
        if k % 8 == 0:
            still_fine()
        else:
            set_case(fx, c)
    assert lib.conp_shake_set_params(fx.h, None) == -1
    _raises(-2, fx.shake_correct_device, X)
    still_fine()
    # the step entries: NULL pointers change nothing -- the next call gives the unrefused result
    set_case(fx, c)
    for a in ((0, V, Fp), (X, 0, Fp), (X, V, 0)):
        _raises(-1, fx.shake_post_force_device, *a, O, VA)
        _raises(-1, fx.shake_setup_device, *a, O)
    _raises(-1, fx.shake_correct_device, 0)
    _raises(-1, fx.shake_check_device, 0, T)
    fx.shake_check_device(X, 0)                                                                 # NULL d_out: nothing done
    assert host(d_x).tobytes() == c.x.tobytes() and host(d_f).tobytes() == c.f.tobytes() and np.isnan(host(d_out)).all()
    assert np.isnan(host(d_va)).all() and np.isnan(host(d_two)).all()
    assert all(p.tobytes() == q.tobytes() for p, q in zip(post_force(fx, c), want))
    # tables without types may be NULL when no cluster refers to them: flag-2 clusters alone need no angle distance
    two = sr.ladder_case(2, 65)
    cl2 = np.ascontiguousarray(two.cluster, dtype=np.int32)
    assert params(nlocal=two.nlocal, type=ip(two.type), ncluster=two.ncluster, cluster=ip(cl2), nangletypes=0, angle_distance=None) == 0
    bare = post_force(fx, two)
    set_case(fx, two)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(bare, post_force(fx, two)))
    compare(two, bare)
    # ncluster == 0: CONP_OK, d_out zeroed, nothing else touched
    fx.shake_set_params(c.type, c.mass, c.bond_d, c.angle_d, np.zeros((0, 7), dtype=np.int32), c.tolerance, c.max_iter, c.dt, c.ftm2v)
    got = post_force(fx, c)
    assert got[0].tobytes() == c.f.tobytes() and not got[1].any() and np.isnan(got[2]).all()
    got = post_force(fx, c, setup=True)
    assert got[0].tobytes() == c.f.tobytes() and not got[1].any()
    fx.shake_correct_device(X)
    fx.shake_check_device(X, T)
    assert host(d_x).tobytes() == c.x.tobytes() and not host(d_two).any()
    # nlocal == 0 as well
    e = np.zeros(0, dtype=np.int32)
    fx.shake_set_params(e, c.mass, c.bond_d, c.angle_d, np.zeros((0, 7), dtype=np.int32), c.tolerance, c.max_iter, c.dt, c.ftm2v)
    fx.shake_post_force_device(X, V, Fp, O, 0)
    assert not host(d_out).any()
    still_fine()
    fx.close()
