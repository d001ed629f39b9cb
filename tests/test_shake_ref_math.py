"""no GPU: the two restatements of the SHAKE rule in tests/shake_ref.py against each other and against what the rule must satisfy,
and the inputs of tests/test_gpu_shake.py against what those tests claim about them."""
import functools
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest

import integrate_ref as ir
import shake_ref as sr

LD = np.longdouble
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lammps-user-conp2_amd", "csrc")


def test_launch_shapes_restated():
    k = open(os.path.join(CSRC, "conp_kernels.h")).read()
    val = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", k).group(1))
    assert (val("SHAKE_BLOCK"), val("SHAKE_FINISH"), val("SHAKE_PART_W")) == (sr.BLOCK, sr.FINISH, 9)
    src = open(os.path.join(CSRC, "conp_shake.hip")).read()
    assert "r += SHAKE_FINISH" in src and "blockIdx.x * SHAKE_BLOCK + threadIdx.x" in src
    assert sr.BIG == sr.BLOCK * sr.FINISH + 1 and sr.BIG <= 100000
    for edge in (1, 63, 64, 65, sr.BLOCK - 1, sr.BLOCK, sr.BLOCK + 1, 1000, sr.BIG):
        assert edge in sr.SIZES


@functools.lru_cache(maxsize=None)
def solved(k):
    """post_force on GPU input k in both number types"""
    c = sr.gpu_cases()[k]
    n = c.nlocal
    L, F = sr.Rule("ld", c), sr.Rule("f64", c)
    return c, L, F, L.solve(c.x[:n], c.v[:n], c.f[:n]), F.solve(c.x[:n], c.v[:n], c.f[:n])


NCASES = len(sr.gpu_cases())


@pytest.mark.parametrize("k", range(NCASES))
def test_the_two_restatements_agree_and_the_input_condition_holds(k):
    c, L, F, a, b = solved(k)
    tol = sr.tol_of(c.ncluster)
    assert sr.frac(c.tag + ": f", b.out, a.out.v, sr.TOL * a.out.m) <= 1.0
    assert sr.frac(c.tag + ": vatom", b.vatom, a.vatom.v, sr.TOL * a.vatom.m) <= 1.0
    va, ma = L.d_out(a)
    vb, _ = F.d_out(b)
    assert sr.frac(c.tag + ": virial", vb[:6], va[:6], tol * ma[:6]) <= 1.0
    assert tuple(va[6:]) == tuple(vb[6:]) and va[6] == 0 and va[7] == 0            # same counts, same largest niter; all converged
    # the input condition: no |l_new - l| of the longdouble run within 1e-9 tolerance of the tolerance, at any iteration of any cluster
    assert sr.clear_of_the_tolerance(L, c.tolerance) > 1e-9
    for flag in a.flags:
        assert np.array_equal(a.flags[flag].niter, b.flags[flag].niter)
    # atoms in no cluster: f as it was, vatom exactly 0
    idle = ~c.member
    assert idle.any() and b.out[idle].tobytes() == c.f[:c.nlocal][idle].tobytes() and not b.vatom[idle].any()
    assert idle.sum() >= 0.09 * c.nlocal


@pytest.mark.parametrize("k", range(NCASES))
def test_the_net_constraint_force_of_a_cluster_is_zero_and_vatom_adds_up(k):
    c, L, F, a, b = solved(k)
    n = c.nlocal
    fc = ir.Mag(a.out.v - c.f[:n], a.out.m)                                        # what the entry added, at f's magnitude
    for row in c.cluster:
        i = row[1:3] if row[0] == 2 else row[1:4]
        assert np.all(np.abs(fc.v[i].sum(axis=0)) <= sr.TOL * fc.m[i].sum(axis=0))
    va, ma = L.d_out(a)
    assert np.all(np.abs(a.vatom.v.sum(axis=0) - va[:6]) <= sr.tol_of(n) * np.maximum(ma[:6], a.vatom.m.sum(axis=0)))


def _deviation_bound(c):
    """what a loop that stopped at |l_new - l| <= tolerance leaves, relative to the distance.  The l it keeps solves the linear part
    exactly for the quad of the PREVIOUS l, so a squared distance is off by quad(l_new) - quad(l_old): six terms q l l, each moved by
    at most |q| (2 |l| + tolerance) tolerance.  |q| <= 2 (1 / 15.04 + 1 / 57.12)^2 r^2 = 0.0142 r^2, r^2 <= 1.1 d^2 (the ratio of the 1-2
    distance to the shorter bond is inside it: r^2 is each constraint's own), |l| <= 1 (asserted): 6 * 0.0142 * 1.1 * 2 = 0.19
    tolerance d^2, and the distance moves by half of that, relatively"""
    return 0.1 * c.tolerance


@pytest.mark.parametrize("flag", [1, 3, 2])
def test_the_constraints_hold_after_correct_and_after_a_step(flag):
    c = sr.ladder_case(flag, 1000)
    n = c.nlocal
    L, F = sr.Rule("ld", c), sr.Rule("f64", c)
    before = L.check(c.x[:n])
    assert before[0] > 100 * _deviation_bound(c)                                   # the input is off by percents
    xl, xf = L.solve(c.x[:n], None, None, correct=True).out, F.solve(c.x[:n], None, None, correct=True).out
    assert sr.frac("correct: x", xf, xl.v, sr.TOL * xl.m) <= 1.0
    left = L.check(xl)
    got = L.check(xf)
    print(f"flag {flag}: deviation {float(before[0]):.3g} -> {float(left[0]):.3g} (bonds), {float(left[1]):.3g} (1-2) after correct")
    assert max(left) <= _deviation_bound(c)
    assert all(g <= l + 1e-12 for g, l in zip(got, left))
    idle = ~c.member
    assert xf[idle].tobytes() == c.x[:n][idle].tobytes()
    # post_force, then the second half of this step and the first of the next with the same forces: x(t + dt) meets the constraints
    ic = SimpleNamespace(type=c.type, group=np.zeros(n, dtype=np.int32), mass=c.mass, style=[0], dof=[3.0 * n], t_period=[100.0],
                         dt=c.dt, ftm2v=c.ftm2v, mvv2e=ir.MVV2E, boltz=ir.BOLTZ)
    dev = []
    for R, x0 in ((L, xl), (F, xf)):
        I = ir.Rule("ld" if R.ld else "f64", ic)
        res = R.solve(x0, c.v[:n], c.f[:n])
        assert all(np.abs(sr._v(q)).max() <= 1.0 for g in res.flags.values() for q in getattr(g, "raw", []))
        f = res.out
        v, _ = I.final(c.v[:n], f)
        x, v = I.initial(x0, v, f, None)
        dev.append(L.check(x))
    print(f"flag {flag}: after a step {float(dev[0][0]):.3g} (bonds), {float(dev[0][1]):.3g} (1-2)")
    # (post_force runs between the two kicks of the SAME force: `final` adds dtf f / m, the next `initial` adds it again and moves x by
    #  dtv v -- x + dtv (v + 2 dtf f / m) = x + dtv v + dtfsq f / m, the position the multipliers were solved for)
    assert max(dev[0]) <= _deviation_bound(c)
    assert all(g <= l + 1e-12 for g, l in zip(dev[1], dev[0]))


@pytest.mark.parametrize("flag", [1, 3])
def test_the_multipliers_solve_the_quadratic_equations(flag):
    """iterated 50 times without a stop: sum_j a_kj l_j + quad_k(l) = d_k^2 - s_k^2 to the bound -- the check of the cofactor and
    quad tables that does not depend on their transcription (the equations are formed here from the constraint itself:
    |s_k + sum of the displacements the multipliers cause|^2 = d_k^2)"""
    c = sr.with_(sr.ladder_case(flag, 1000), max_iter=50, tolerance=1e-300)
    n = c.nlocal
    L = sr.Rule("ld", c)
    res = L.solve(c.x[:n], c.v[:n], c.f[:n])
    assert res.niter_max > sr.MAX_ITER                  # (most clusters reach a fixed point of the longdouble arithmetic before 50)
    g = res.flags[flag]
    # the constraint itself: move xs by dtfmsq_k fc_k and measure
    xs = c.x[:n].astype(LD) + LD(c.dt) * c.v[:n].astype(LD) + (L.dtfsq(False).v / c.mass[c.type - 1].astype(LD))[:, None] * res.out.v
    worst = 0.0
    for row in c.cluster:
        pairs = [(1, 2, c.bond_d[0]), (1, 3, c.bond_d[1])] + ([(2, 3, c.angle_d[0])] if flag == 1 else [])
        for i, j, d in pairs:
            r = xs[row[i]] - xs[row[j]]
            worst = max(worst, float(abs(np.sqrt((r * r).sum()) - d) / d))
    print(f"flag {flag}: largest deviation with converged multipliers {worst:.3g}")
    assert worst <= 1e-12
    # and the equations term by term, with the magnitudes the reference carries
    K = len(g.raw)
    pairs = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)] if K == 3 else [(0, 0), (1, 1), (0, 1)]
    for k in range(K):
        lhs = g.a[k][0] * g.raw[0]
        for j in range(1, K):
            lhs = lhs + g.a[k][j] * g.raw[j]
        for q, (i, j) in zip(g.quads[k], pairs):
            lhs = lhs + q * g.raw[i] * g.raw[j]
        rhs = g.dsq[k] - g.ssq[k]
        assert np.all(np.abs(lhs.v - rhs.v) <= sr.TOL * (lhs.m + rhs.m))


def test_setup_is_post_force_at_half_dtfsq():
    c = sr.mixed_case()
    n = c.nlocal
    F = sr.Rule("f64", c)
    a, b = F.solve(c.x[:n], c.v[:n], c.f[:n]), F.solve(c.x[:n], c.v[:n], c.f[:n], half=True)
    fa, fb = (a.out - c.f[:n])[c.member], (b.out - c.f[:n])[c.member]
    assert np.all(fa != fb) and float(F.dtfsq(True)) * 2 == float(F.dtfsq(False))


def test_the_cases_contain_what_the_gpu_tests_claim():
    for c in sr.gpu_cases():
        n = c.nlocal
        assert c.x.shape == c.v.shape == c.f.shape == (n + sr.SENTINELS, 3) and c.cluster.shape == (c.ncluster, 7)
        used = np.concatenate([row[1:3] if row[0] == 2 else row[1:4] for row in c.cluster])
        assert len(set(used)) == len(used) and used.min() >= 0 and used.max() < n and c.member.sum() == len(used)
        assert (~c.member).sum() >= 1
        if c.ncluster >= 63:                                                      # permuted: the members of a cluster are not neighbours
            first = c.cluster[:, 1].astype(np.int64)
            assert np.abs(c.cluster[:, 2] - first).max() > c.ncluster // 2 and not np.all(np.diff(first) > 0)
        for row in c.cluster:                                                     # fields a flag does not use hold junk
            if row[0] == 2:
                assert row[3] == -7 and row[5] == 99 and row[6] == 99
            if row[0] == 3:
                assert row[6] == 99
    m = sr.mixed_case()
    assert set(m.cluster[:, 0]) == {1, 2, 3} and len(set(m.cluster[:20, 0])) == 3
    for w in ("x", "y", "z", "xyz"):
        c = sr.straddle_case(w)
        u = sr.unwrapped(c)
        for ch in w:
            k = "xyz".index(ch)
            span = np.array([np.ptp(c.x[row[1:4], k]) for row in c.cluster])
            assert (span > 20.0).sum() >= 4                                       # members on both sides of the box
            assert np.array([np.ptp(u.x[row[1:4], k]) for row in u.cluster]).max() < 6.0
        assert c.x[:c.nlocal].min() >= 0.0 and c.x[:c.nlocal].max() < 40.0 and not u.prd.any()


def _condition(c, x=None, **how):
    """one solve in both number types -> (longdouble result, float64 result); asserts the input condition and equal iteration counts"""
    n = c.nlocal
    L, F = sr.Rule("ld", c), sr.Rule("f64", c)
    x = c.x[:n] if x is None else x
    a, b = L.solve(x, c.v[:n], c.f[:n], **how), F.solve(x, c.v[:n], c.f[:n], **how)
    assert sr.clear_of_the_tolerance(L, c.tolerance) > 1e-9, c.tag
    assert all(np.array_equal(a.flags[k].niter, b.flags[k].niter) for k in a.flags)
    assert sr.frac(c.tag, b.out, a.out.v, sr.TOL * a.out.m) <= 1.0
    return a, b


def test_the_input_condition_on_the_remaining_gpu_inputs():
    """what tests/test_gpu_shake.py runs beside gpu_cases(): setup and correct on the mixed case, the deck (correct, then post_force
    from the corrected x), the loops cut short, the constructed determinants, and every solve of the two device-step runs"""
    m = sr.mixed_case()
    _condition(m, half=True)
    _condition(m, correct=True)
    d = sr.deck_case()
    assert d.ncluster == 320 and d.nlocal == 3776 and np.all(d.cluster[:, 0] == 1) and d.prd[2] == 0 and d.prd[0] > 0
    span = np.array([np.ptp(d.x[row[1:4]], axis=0) for row in d.cluster])
    assert (span[:, 0] > 20).any() and (span[:, 1] > 20).any()                    # molecules split across the box in x and in y
    _, xf = _condition(d, correct=True)
    _condition(d, x=xf.out)
    for max_iter in (1, 2):
        s = sr.strong_case(max_iter)
        a, _ = _condition(s)
        assert a.unconverged == s.ncluster and a.niter_max == max_iter
    sp = sr.special_case()
    a, b = _condition(sp)
    assert a.bad_determ == b.bad_determ == 3 and a.unconverged == 0
    rows = sp.cluster[sp.first_special:]
    assert list(rows[:, 0]) == [3, 1, 2]
    for row in rows[:2]:                                                          # determ == 0: nothing added, vatom 0
        assert b.out[row[1:4]].tobytes() == sp.f[row[1:4]].tobytes() and not b.vatom[row[1:4]].any()
    _condition(sp, correct=True)
    for style in (0, 1):
        c = sr.step_case(style)
        r = sr.reference_steps(c)
        assert r.near > 1e-9 and tuple(r.shake[0][6:8]) == (0, 0)
        assert len(c.angles) == (c.cluster[:, 0] == 3).sum() > 10 and set(c.cluster[:, 0]) == {1, 2, 3}
        assert max(float(q) for dev in r.check for q in dev) <= _deviation_bound(c)
