"""-m gpu: the conp_integrate_* entries -- velocity Verlet and the Nose-Hoover chain -- against the
restatements of tests/integrate_ref.py: the nve path bit for bit against float64 in the written order (no transcendental, no sum
in it), everything else entry-wise to 1e-12 of the longdouble reference's cancellation-free magnitude (n 2^-53 for the one case
with more than 2^13 atoms).  x, v and f carry 64 sentinel rows behind nlocal, and every case has atoms in no group: all of these
stay bit for bit.  Then a sequence of steps without a synchronisation, its repetition and its continuation on a second handle, a
whole device step with the bonded term, mixed styles, and the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

from conp_amd import ConpError, FixConp, capi, systems
import bonded_ref as br
import integrate_ref as ir

pytestmark = pytest.mark.gpu
LD = np.longdouble


@functools.lru_cache(maxsize=None)
def handle():
    """one handle for most cases: the entries need nothing of the fix but its stream, and no setup call is made on it"""
    return FixConp(systems.small_random(ne_side=4, n_elyte=64))


def set_case(fx, c):
    fx.integrate_set_params(c.type, c.group, c.mass, c.style, c.dof, c.t_period, c.dt, c.ftm2v, c.mvv2e, c.boltz)


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).cuda()


def out_tensor(c):
    import torch
    return torch.full((len(c.style), 4), float("nan"), dtype=torch.float64, device="cuda")


def host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def untouched(c, got, start):
    """the sentinel rows and the rows of atoms in no group, bit for bit"""
    idle = np.concatenate([c.group == -1, np.full(ir.SENTINELS, True)])
    return got[idle].tobytes() == start[idle].tobytes()


class Worst(dict):
    def note(self, key, fr):
        self[key] = max(self.get(key, 0.0), fr)

    def line(self, tag):
        print(f"{tag}: largest fraction of the bound: " + ", ".join(f"{k} {v:.3g}" for k, v in self.items()))
        assert max(self.values()) <= 1.0, (tag, dict(self))


def check_out(w, tag, key, got, rows, tol):
    val, mag = ir.out_arrays(rows)
    w.note(key, ir.frac(f"{tag}: {key}", got, val, tol * mag))


def check_state(w, tag, fx, R, tol):
    val, mag = R.get_state()
    w.note("state", ir.frac(f"{tag}: state", fx.integrate_get_state(), val, tol * mag))


# ---- nve: bit for bit ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", ir.SIZES + (ir.BIG,))
def test_nve_is_the_float64_restatement_bit_for_bit(n):
    """every block edge, and BIG = INTEGRATE_BLOCK * INTEGRATE_FINISH + 1 = 65537 atoms: 257 rows of partial sums, one more than
    the 256 threads of the finishing workgroup take in one round"""
    c = ir.nve_case(n)
    fx = handle()
    set_case(fx, c)
    F, L = ir.Rule("f64", c), ir.Rule("ld", c)
    d_x, d_v, d_f, d_f2, d_out = dev(c.x), dev(c.v), dev(c.f), dev(ir.fresh_forces(c, 1)), out_tensor(c)
    fx.integrate_initial_device(d_x.data_ptr(), d_v.data_ptr(), d_f.data_ptr(), c.t_target)    # no setup: no nvt group
    x1, v1 = host(d_x), host(d_v)
    xr, vr = F.initial(c.x[:n], c.v[:n], c.f[:n], None)
    assert x1[:n].tobytes() == xr.tobytes() and v1[:n].tobytes() == vr.tobytes()
    assert untouched(c, x1, c.x) and untouched(c, v1, c.v)
    fx.integrate_final_device(d_v.data_ptr(), d_f2.data_ptr(), d_out.data_ptr())
    v2, out = host(d_v), host(d_out)
    f2 = ir.fresh_forces(c, 1)[:n]
    vr2, _ = F.final(vr, f2)
    assert v2[:n].tobytes() == vr2.tobytes() and untouched(c, v2, c.v) and host(d_x).tobytes() == x1.tobytes()
    _, rows = L.final(vr, f2)
    w = Worst()
    check_out(w, c.tag, "d_out", out, rows, ir.tol_of(n))
    assert not out[:, 2:].any() and not np.signbit(out[:, 2:]).any()                           # nve: exactly 0.0
    d_t = out_tensor(c)
    fx.integrate_temperature_device(d_v.data_ptr(), d_t.data_ptr())
    assert host(d_t).tobytes() == out.tobytes()                                                # the same sums in the same order
    w.line(c.tag)


# ---- nvt: each entry from a seeded state ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("build", [ir.nvt_one, ir.nvt_two, ir.nvt_eight, ir.nvt_big], ids=lambda b: b.__name__)
def test_nvt_entries_from_a_seeded_state(build):
    c = build()
    n, tol = c.nlocal, ir.tol_of(c.nlocal)
    fx = handle()
    set_case(fx, c)
    w = Worst()
    f2 = ir.fresh_forces(c, 1)
    # temperature: the sums of d_v and the chain as seeded; nothing is stored
    fx.integrate_set_state(c.state0)
    R = ir.Rule("ld", c); R.set_state(c.state0)
    d_v, d_out = dev(c.v), out_tensor(c)
    fx.integrate_temperature_device(d_v.data_ptr(), d_out.data_ptr())
    check_out(w, c.tag, "temperature", host(d_out), R.temperature(c.v[:n]), tol)
    assert host(d_v).tobytes() == c.v.tobytes()
    assert fx.integrate_get_state().tobytes() == np.ascontiguousarray(c.state0).tobytes()
    for g in np.nonzero(c.count == 0)[0]:
        assert not host(d_out)[g, :2].any()                                                    # a group without atoms: exactly 0.0
    # setup: t_current and t_target stored, eta and eta_dot kept
    fx.integrate_setup_device(d_v.data_ptr(), c.t_target + 1.0)
    R.setup(c.v[:n], c.t_target + 1.0)
    check_state(w, c.tag + ", setup", fx, R, tol)
    assert host(d_v).tobytes() == c.v.tobytes()
    # initial from the seeded state
    fx.integrate_set_state(c.state0)
    R = ir.Rule("ld", c); R.set_state(c.state0)
    d_x, d_v, d_f = dev(c.x), dev(c.v), dev(c.f)
    fx.integrate_initial_device(d_x.data_ptr(), d_v.data_ptr(), d_f.data_ptr(), c.t_target)
    xr, vr = R.initial(c.x[:n], c.v[:n], c.f[:n], c.t_target)
    x1, v1 = host(d_x), host(d_v)
    w.note("x", ir.frac(f"{c.tag}, initial: x", x1[:n], xr.v, tol * xr.m))
    w.note("v", ir.frac(f"{c.tag}, initial: v", v1[:n], vr.v, tol * vr.m))
    assert untouched(c, x1, c.x) and untouched(c, v1, c.v) and host(d_f).tobytes() == c.f.tobytes()
    check_state(w, c.tag + ", initial", fx, R, tol)
    # final from the seeded state
    fx.integrate_set_state(c.state0)
    R = ir.Rule("ld", c); R.set_state(c.state0)
    d_v, d_f, d_out = dev(c.v), dev(f2), out_tensor(c)
    fx.integrate_final_device(d_v.data_ptr(), d_f.data_ptr(), d_out.data_ptr())
    vr, rows = R.final(c.v[:n], f2[:n])
    v1 = host(d_v)
    w.note("v", ir.frac(f"{c.tag}, final: v", v1[:n], vr.v, tol * vr.m))
    check_out(w, c.tag + ", final", "d_out", host(d_out), rows, tol)
    assert untouched(c, v1, c.v)
    check_state(w, c.tag + ", final", fx, R, tol)
    # the same call without d_out: the same velocities and state
    st = fx.integrate_get_state()
    fx.integrate_set_state(c.state0)
    d_v2 = dev(c.v)
    fx.integrate_final_device(d_v2.data_ptr(), d_f.data_ptr(), 0)
    assert host(d_v2).tobytes() == v1.tobytes() and fx.integrate_get_state().tobytes() == st.tobytes()
    w.line(c.tag)


# ---- a sequence ------------------------------------------------------------------------------------------------------------------------
STEPS = 5


def run_sequence(fx, c, forces, first, last, x, v, with_setup):
    """steps first .. last-1 of initial -> final enqueued with nothing between; ONE synchronisation behind the last
    -> (x, v, d_out of every step, the state)"""
    import torch
    d_x, d_v = dev(x), dev(v)
    outs = [out_tensor(c) for _ in range(first, last)]
    torch.cuda.synchronize()
    if with_setup:
        fx.integrate_setup_device(d_v.data_ptr(), c.t_target)
    for k, s in enumerate(range(first, last)):
        fx.integrate_initial_device(d_x.data_ptr(), d_v.data_ptr(), forces[2 * s].data_ptr(), c.t_target + s)
        fx.integrate_final_device(d_v.data_ptr(), forces[2 * s + 1].data_ptr(), outs[k].data_ptr())
    torch.cuda.synchronize()
    return d_x.cpu().numpy(), d_v.cpu().numpy(), [o.cpu().numpy() for o in outs], fx.integrate_get_state()


def same(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[3].tobytes() == b[3].tobytes() and \
        all(p.tobytes() == q.tobytes() for p, q in zip(a[2], b[2]))


def test_a_sequence_of_steps_its_repetition_and_its_continuation():
    """5 steps on the 8-group case with a fresh random d_f per half-step and a ramping target; the bound is 1e-12 of the
    magnitudes the reference accumulates.  The run is repeated byte for byte, and a second handle seeded with get_state after
    step 2 continues byte for byte"""
    c = ir.nvt_eight()
    n, tol = c.nlocal, ir.tol_of(c.nlocal)
    fx = handle()
    fh = [ir.fresh_forces(c, s) for s in range(2 * STEPS)]
    forces = [dev(f) for f in fh]
    set_case(fx, c)
    a = run_sequence(fx, c, forces, 0, STEPS, c.x, c.v, True)
    R = ir.Rule("ld", c)
    R.setup(c.v[:n], c.t_target)
    x, v = c.x[:n], c.v[:n]
    w = Worst()
    for s in range(STEPS):
        x, v = R.initial(x, v, fh[2 * s][:n], c.t_target + s)
        v, rows = R.final(v, fh[2 * s + 1][:n])
        check_out(w, f"step {s}", "d_out", a[2][s], rows, tol)
    w.note("x", ir.frac("5 steps: x", a[0][:n], x.v, tol * x.m))
    w.note("v", ir.frac("5 steps: v", a[1][:n], v.v, tol * v.m))
    val, mag = R.get_state()
    w.note("state", ir.frac("5 steps: state", a[3], val, tol * mag))
    assert untouched(c, a[0], c.x) and untouched(c, a[1], c.v)
    moved = np.abs(a[0][:n] - c.x[:n])[c.group >= 0]
    assert np.median(moved) > 1e6 * float(np.median(tol * x.m))                                 # the atoms went somewhere
    w.line("a sequence of 5 steps, 8 groups")
    set_case(fx, c)                                                                            # zeroes every chain
    assert not fx.integrate_get_state().any()
    assert same(run_sequence(fx, c, forces, 0, STEPS, c.x, c.v, True), a)
    # two steps here, the state handed to a second handle, the rest there
    set_case(fx, c)
    head = run_sequence(fx, c, forces, 0, 2, c.x, c.v, True)
    fx2 = FixConp(systems.small_random(ne_side=4, n_elyte=64))
    set_case(fx2, c)
    fx2.integrate_set_state(head[3])
    tail = run_sequence(fx2, c, forces, 2, STEPS, head[0], head[1], False)
    assert tail[0].tobytes() == a[0].tobytes() and tail[1].tobytes() == a[1].tobytes() and tail[3].tobytes() == a[3].tobytes()
    assert all(p.tobytes() == q.tobytes() for p, q in zip(head[2] + tail[2], a[2]))
    fx2.close()


# ---- a device step ----------------------------------------------------------------------------------------------------------------------
def test_three_device_steps_with_the_bonded_term():
    """the closest-image molecules of tests/bonded_ref.py: integrate_initial -> zero d_f -> bonded_compute_device -> integrate_final,
    three times on one stream without a synchronisation, against the longdouble integrator driven by bonded_ref's forces"""
    import torch
    b = br.molecules(True, "image")
    n = b.nlocal
    assert b.nall == n
    elyte = b.s.echeck[:n] == 0
    group = np.where(elyte, 0, -1).astype(np.int32)
    ntypes = int(b.s.type.max())
    mass = np.resize(ir.MASS[:4], ntypes)
    rng = np.random.default_rng(77)
    m_atom = mass[b.s.type[:n] - 1]
    v0 = rng.normal(size=(n, 3)) * np.sqrt(ir.BOLTZ * 400.0 / (m_atom * ir.MVV2E))[:, None]
    c = ir.SimpleNamespace(tag="device step", nlocal=n, type=b.s.type[:n].astype(np.int32), group=group, mass=mass,
                           style=np.array([1], dtype=np.int32), dof=np.array([3.0 * elyte.sum() - 3.0]), t_period=np.array([100.0]), dt=1.0,
                           ftm2v=ir.FTM2V, mvv2e=ir.MVV2E, boltz=ir.BOLTZ, t_target=np.array([400.0]))
    fx = FixConp(systems.small_random(ne_side=4, n_elyte=64))
    fx.set_stream(torch.cuda.current_stream().cuda_stream)                   # torch's zero_() and the entries on ONE stream
    set_case(fx, c)
    fx.bonded_set_params(b.p.bond_k, b.p.bond_r0, b.p.angle_k, b.p.angle_theta0, newton_bond=True)
    fx.bonded_set_lists(n, n, b.bonds, b.angles, b.prd)
    f0 = br.reference(b.x, n, b.bonds, b.angles, b.p, True, b.prd)
    d_x, d_v, d_f, d_out = dev(b.x), dev(v0), dev(f0.f.astype(np.float64)), out_tensor(c)
    torch.cuda.synchronize()
    fx.integrate_setup_device(d_v.data_ptr(), c.t_target)
    for _ in range(3):
        fx.integrate_initial_device(d_x.data_ptr(), d_v.data_ptr(), d_f.data_ptr(), c.t_target)
        d_f.zero_()
        fx.bonded_compute_device(d_x.data_ptr(), d_f.data_ptr(), 0, 0, 0)
        fx.integrate_final_device(d_v.data_ptr(), d_f.data_ptr(), d_out.data_ptr())
    torch.cuda.synchronize()
    R = ir.Rule("ld", c)
    R.setup(v0, c.t_target)
    x, v, f = b.x, v0, ir.Mag(f0.f, f0.A)
    for _ in range(3):
        x, v = R.initial(x, v, f, c.t_target)
        fr = br.reference(x.v.astype(np.float64), n, b.bonds, b.angles, b.p, True, b.prd)
        f = ir.Mag(fr.f, fr.A)
        v, rows = R.final(v, f)
    w = Worst()
    # (the reference's forces are those of its x rounded to float64: the device's x differs from it by rounding, which a spring
    #  constant of 553 turns into 1e-12 kcal/mol/A beside magnitudes of 1e3: inside the bound)
    w.note("x", ir.frac("3 device steps: x", d_x.cpu().numpy(), x.v, ir.TOL * x.m))
    w.note("v", ir.frac("3 device steps: v", d_v.cpu().numpy(), v.v, ir.TOL * v.m))
    check_out(w, "3 device steps", "d_out", d_out.cpu().numpy(), rows, ir.TOL)
    check_state(w, "3 device steps", fx, R, ir.TOL)
    moved = np.abs(d_x.cpu().numpy() - b.x)
    assert moved[elyte].min() > 0 and np.median(moved[elyte]) > 1e6 * float(np.median(ir.TOL * x.m)) and not moved[~elyte].any()
    w.line("3 device steps with the bonded term")
    fx.close()


# ---- mixed styles ------------------------------------------------------------------------------------------------------------------------
def test_an_nve_group_beside_an_nvt_group_moves_as_it_does_alone():
    c = ir.mixed()
    n = c.nlocal
    fx = handle()
    res = []
    for case in (c, ir.as_nve(c)):
        set_case(fx, case)
        d_x, d_v, d_f, d_f2 = dev(c.x), dev(c.v), dev(c.f), dev(ir.fresh_forces(c, 1))
        fx.integrate_setup_device(d_v.data_ptr(), c.t_target)
        for _ in range(2):
            fx.integrate_initial_device(d_x.data_ptr(), d_v.data_ptr(), d_f.data_ptr(), c.t_target)
            fx.integrate_final_device(d_v.data_ptr(), d_f2.data_ptr(), 0)
        res.append((host(d_x)[:n], host(d_v)[:n]))
    nve, nvt = c.group == 0, c.group == 1
    assert res[0][0][nve].tobytes() == res[1][0][nve].tobytes() and res[0][1][nve].tobytes() == res[1][1][nve].tobytes()
    assert np.all(res[0][1][nvt] != res[1][1][nvt])                                            # ... and the thermostat acts on the other
    R = ir.Rule("ld", c)
    R.setup(c.v[:n], c.t_target)
    x, v = c.x[:n], c.v[:n]
    for _ in range(2):
        x, v = R.initial(x, v, c.f[:n], c.t_target)
        v, _ = R.final(v, ir.fresh_forces(c, 1)[:n])
    w = Worst()
    w.note("x", ir.frac("mixed: x", res[0][0], x.v, ir.TOL * x.m))
    w.note("v", ir.frac("mixed: v", res[0][1], v.v, ir.TOL * v.m))
    w.line(c.tag)


# ---- refusals -----------------------------------------------------------------------------------------------------------------------------
def _raises(code, fn, *a, **k):
    with pytest.raises(ConpError) as e:
        fn(*a, **k)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_refusals_and_special_cases():
    c = ir.nvt_two()
    n = c.nlocal
    fx = FixConp(systems.small_random(ne_side=4, n_elyte=64))
    lib = fx.lib
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    mass1 = np.concatenate([[0.0], c.mass])
    d_f2 = dev(ir.fresh_forces(c, 1))

    def step():
        """setup and one step from the case's start -> (x, v, d_out, state)"""
        d_x, d_v, d_f, d_out = dev(c.x), dev(c.v), dev(c.f), out_tensor(c)
        fx.integrate_setup_device(d_v.data_ptr(), c.t_target)
        fx.integrate_initial_device(d_x.data_ptr(), d_v.data_ptr(), d_f.data_ptr(), c.t_target)
        fx.integrate_final_device(d_v.data_ptr(), d_f2.data_ptr(), d_out.data_ptr())
        return host(d_x), host(d_v), host(d_out), fx.integrate_get_state()

    def params(**k):
        v = dict(nlocal=n, ntypes=len(c.mass), ngroups=2, type=ip(c.type), group=ip(c.group), mass=dp(mass1), style=ip(c.style),
                 dof=dp(c.dof), t_period=dp(c.t_period), dt=c.dt, ftm2v=c.ftm2v, mvv2e=c.mvv2e, boltz=c.boltz)
        v.update(k)
        return lib.conp_integrate_set_params(fx.h, C.byref(capi.conp_integrate_params(**v)))
    d_x, d_v, d_f, d_out = dev(c.x), dev(c.v), dev(c.f), out_tensor(c)
    X, V, Fp, O = d_x.data_ptr(), d_v.data_ptr(), d_f.data_ptr(), d_out.data_ptr()
    st8 = np.zeros((2, 8))
    # before set_params: every other entry is out of order
    for call in (lambda: lib.conp_integrate_setup_device(fx.h, V, dp(c.t_target)),
                 lambda: lib.conp_integrate_initial_device(fx.h, X, V, Fp, dp(c.t_target)),
                 lambda: lib.conp_integrate_final_device(fx.h, V, Fp, O), lambda: lib.conp_integrate_temperature_device(fx.h, V, O),
                 lambda: lib.conp_integrate_get_state(fx.h, dp(st8)), lambda: lib.conp_integrate_set_state(fx.h, dp(st8))):
        assert call() == -2
    set_case(fx, c)
    # initial and final before setup with an nvt group
    _raises(-2, fx.integrate_initial_device, X, V, Fp, c.t_target)
    _raises(-2, fx.integrate_final_device, V, Fp, O)
    fx.integrate_temperature_device(V, O)                                                       # (needs no setup)
    want = step()
    w = Worst()
    R = ir.Rule("ld", c); R.setup(c.v[:n], c.t_target)
    xr, vr = R.initial(c.x[:n], c.v[:n], c.f[:n], c.t_target)
    vr, rows = R.final(vr, ir.fresh_forces(c, 1)[:n])
    w.note("x", ir.frac("before the refusals: x", want[0][:n], xr.v, ir.TOL * xr.m))
    w.note("v", ir.frac("before the refusals: v", want[1][:n], vr.v, ir.TOL * vr.m))
    check_out(w, "before the refusals", "d_out", want[2], rows, ir.TOL)
    w.line("before the refusals")

    def still_fine():
        set_case(fx, c)
        got = step()
        assert all(g.tobytes() == h.tobytes() for g, h in zip(got, want))
    # set_params: each refusal leaves the handle without an integrator; a valid call gives the unrefused result again
    nan, inf = float("nan"), float("inf")
    t_hi, t_0, g_hi, g_lo = c.type.copy(), c.type.copy(), c.group.copy(), c.group.copy()
    t_hi[5] = len(c.mass) + 1; t_0[7] = 0; g_hi[3] = 2; g_lo[9] = -2
    m_0, m_neg, m_nan, m_inf = (mass1.copy() for _ in range(4))
    m_0[2] = 0.0; m_neg[1] = -1.0; m_nan[3] = nan; m_inf[5] = inf
    dof_0, dof_nan, tp_0, tp_inf = c.dof.copy(), c.dof.copy(), c.t_period.copy(), c.t_period.copy()
    dof_0[1] = 0.0; dof_nan[0] = nan; tp_0[0] = 0.0; tp_inf[1] = inf
    style_2 = np.array([1, 2], dtype=np.int32)
    refused = [dict(type=None), dict(group=None), dict(mass=None), dict(style=None), dict(dof=None), dict(t_period=None),
               dict(ngroups=0), dict(ngroups=ir.MAX_GROUPS + 1), dict(nlocal=-1),
               dict(type=ip(t_hi)), dict(type=ip(t_0)), dict(group=ip(g_hi)), dict(group=ip(g_lo)), dict(style=ip(style_2)),
               dict(mass=dp(m_0)), dict(mass=dp(m_neg)), dict(mass=dp(m_nan)), dict(mass=dp(m_inf)),
               dict(dt=0.0), dict(dt=-1.0), dict(dt=nan), dict(ftm2v=0.0), dict(ftm2v=inf), dict(mvv2e=-1.0), dict(mvv2e=nan),
               dict(boltz=0.0), dict(boltz=inf), dict(dof=dp(dof_0)), dict(dof=dp(dof_nan)), dict(t_period=dp(tp_0)), dict(t_period=dp(tp_inf))]
    for k, bad in enumerate(refused):
        assert params(**bad) == -1, bad
        _raises(-2, fx.integrate_temperature_device, V, O)
        assert lib.conp_integrate_get_state(fx.h, dp(st8)) == -2
        if k % 6 == 0:
            still_fine()
        else:
            set_case(fx, c)
    assert lib.conp_integrate_set_params(fx.h, None) == -1
    _raises(-2, fx.integrate_final_device, V, Fp, O)
    still_fine()
    # the step entries: NULL pointers and bad targets change nothing -- the next calls give the unrefused step
    set_case(fx, c)
    d_x, d_v, d_f = dev(c.x), dev(c.v), dev(c.f)
    X, V, Fp = d_x.data_ptr(), d_v.data_ptr(), d_f.data_ptr()
    bad_targets = [np.array([-1.0, 400.0]), np.array([400.0, nan]), np.array([inf, 400.0]), np.array([400.0, 0.0])]
    _raises(-1, fx.integrate_setup_device, 0, c.t_target)
    _raises(-1, fx.integrate_setup_device, V, None)
    for t in bad_targets:
        _raises(-1, fx.integrate_setup_device, V, t)
    _raises(-2, fx.integrate_initial_device, X, V, Fp, c.t_target)                              # a refused setup is no setup
    fx.integrate_setup_device(V, c.t_target)
    for a in ((0, V, Fp), (X, 0, Fp), (X, V, 0)):
        _raises(-1, fx.integrate_initial_device, *a, c.t_target)
    _raises(-1, fx.integrate_initial_device, X, V, Fp, None)
    for t in bad_targets:
        _raises(-1, fx.integrate_initial_device, X, V, Fp, t)
    fx.integrate_initial_device(X, V, Fp, c.t_target)
    _raises(-1, fx.integrate_final_device, 0, d_f2.data_ptr(), O)
    _raises(-1, fx.integrate_final_device, V, 0, O)
    _raises(-1, fx.integrate_temperature_device, 0, O)
    fx.integrate_temperature_device(V, 0)                                                       # NULL d_out: nothing done
    fx.integrate_final_device(V, d_f2.data_ptr(), O)
    got = (host(d_x), host(d_v), host(d_out), fx.integrate_get_state())
    assert all(g.tobytes() == h.tobytes() for g, h in zip(got, want))
    # the state entries
    assert lib.conp_integrate_get_state(fx.h, None) == -1 and lib.conp_integrate_set_state(fx.h, None) == -1
    for col, val in ((0, nan), (4, inf), (6, nan), (7, -1.0), (7, 0.0), (7, inf)):
        s = want[3].copy(); s[1, col] = val
        _raises(-1, fx.integrate_set_state, s)
    assert fx.integrate_get_state().tobytes() == want[3].tobytes()
    # nlocal == 0: CONP_OK, d_out zeroed
    e = np.zeros(0, dtype=np.int32)
    fx.integrate_set_params(e, e, c.mass, c.style, c.dof, c.t_period, c.dt, c.ftm2v, c.mvv2e, c.boltz)
    fx.integrate_setup_device(V, c.t_target)
    fx.integrate_initial_device(X, V, Fp, c.t_target)
    d_o2 = out_tensor(c)
    fx.integrate_final_device(V, Fp, d_o2.data_ptr())
    assert not host(d_o2).any()
    d_o2 = out_tensor(c)
    fx.integrate_temperature_device(V, d_o2.data_ptr())
    assert not host(d_o2).any() and host(d_v).tobytes() == want[1].tobytes() and host(d_x).tobytes() == want[0].tobytes()
    still_fine()
    fx.close()
