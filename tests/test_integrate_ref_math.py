"""no GPU: the two restatements of the integration rule in tests/integrate_ref.py against each other and against what the rule
must satisfy, and the inputs of tests/test_gpu_integrate.py against what those tests claim about them."""
import os
import re

import numpy as np
import pytest

import integrate_ref as ir

LD = np.longdouble
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lammps-user-conp2_amd", "csrc")


def test_launch_shapes_restated():
    """integrate_ref restates the launch shapes of conp_integrate.hip: whoever changes one there is sent here"""
    k = open(os.path.join(CSRC, "conp_kernels.h")).read()
    val = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", k).group(1))
    assert (val("INTEGRATE_BLOCK"), val("INTEGRATE_FINISH")) == (ir.BLOCK, ir.FINISH)
    hdr = open(os.path.join(CSRC, "..", "..", "include", "conp_hip.h")).read()
    assert int(re.search(r"#define CONP_INTEGRATE_MAX_GROUPS (\d+)", hdr).group(1)) == ir.MAX_GROUPS
    assert int(re.search(r"#define CONP_INTEGRATE_CHAIN (\d+)", hdr).group(1)) == 3
    src = open(os.path.join(CSRC, "conp_integrate.hip")).read()
    assert "r += INTEGRATE_FINISH" in src and "blockIdx.x * INTEGRATE_BLOCK + threadIdx.x" in src
    assert ir.BIG == ir.BLOCK * ir.FINISH + 1 and ir.BIG <= 300000


def _both(c):
    return ir.Rule("ld", c), ir.Rule("f64", c)


@pytest.mark.parametrize("build", [ir.nvt_one, ir.nvt_two, ir.nvt_eight, ir.mixed], ids=lambda b: b.__name__)
def test_the_two_restatements_agree(build):
    """setup, then two steps from the seeded state: float64 in the written order stays within the GPU tests' bound of the
    longdouble values, every entry of x, v, d_out and the state"""
    c = build()
    n = c.nlocal
    L, F = _both(c)
    worst = 0.0
    for R in (L, F):
        R.set_state(c.state0)
    tl, tf = L.temperature(c.v[:n]), F.temperature(c.v[:n])
    val, mag = ir.out_arrays(tl)
    worst = max(worst, ir.frac("temperature", np.array(tf, dtype=np.float64), val, ir.tol_of(n) * mag))
    for R in (L, F):
        R.setup(c.v[:n], c.t_target)
    xl, vl, xf, vf = c.x[:n], c.v[:n], c.x[:n], c.v[:n]
    for step in range(2):
        f = ir.fresh_forces(c, step)[:n]
        xl, vl = L.initial(xl, vl, f, c.t_target)
        xf, vf = F.initial(xf, vf, f, c.t_target)
        f = ir.fresh_forces(c, step + 100)[:n]
        vl, ol = L.final(vl, f)
        vf, of = F.final(vf, f)
        val, mag = ir.out_arrays(ol)
        worst = max(worst, ir.frac(f"step {step}: d_out", np.array(of, dtype=np.float64), val, ir.tol_of(n) * mag))
        worst = max(worst, ir.frac(f"step {step}: v", vf, vl.v, ir.tol_of(n) * vl.m), ir.frac(f"step {step}: x", xf, xl.v, ir.tol_of(n) * xl.m))
        sv, sm = L.get_state()
        worst = max(worst, ir.frac(f"step {step}: state", F.get_state()[0], sv, ir.tol_of(n) * sm))
    assert worst <= 1.0
    # ke of the row is the kinetic energy of the velocities the entry leaves, to the bound
    for g in range(len(c.style)):
        w = vl.v[c.group == g]
        direct = (0.5 * LD(c.mvv2e) * ((w * w).sum(axis=1) * np.concatenate([[0.0], c.mass])[c.type][c.group == g].astype(LD)).sum())
        assert abs(direct - val[g, 1]) <= ir.tol_of(n) * mag[g, 1]
    # atoms in no group never move
    idle = c.group == -1
    assert idle.any() and xf[idle].tobytes() == c.x[:n][idle].tobytes() and vf[idle].tobytes() == c.v[:n][idle].tobytes()
    assert np.array_equal(xl.v[idle], c.x[:n][idle].astype(LD))


def test_an_nve_step_is_time_reversible_to_rounding():
    """initial, final; v -> -v; initial, final with the same forces: back at the start with -v, to the accumulated bound"""
    c = ir.nve_case(1000)
    n = c.nlocal
    L, F = _both(c)
    for R, name in ((L, "ld"), (F, "f64")):
        x, v = R.initial(c.x[:n], c.v[:n], c.f[:n], None)
        v, _ = R.final(v, c.f[:n])
        x1 = x
        x, v = R.initial(x, -v, c.f[:n], None)
        v, _ = R.final(v, c.f[:n])
        if name == "ld":
            bound_x, bound_v = ir.TOL * x.m, ir.TOL * v.m
            assert ir.frac("reversed x (ld)", x.v, c.x[:n].astype(LD), bound_x) <= 1.0
            assert ir.frac("reversed v (ld)", -v.v, c.v[:n].astype(LD), bound_v) <= 1.0
            moved = np.abs(x1.v - c.x[:n])[c.group >= 0]
            assert moved.min() > 0 and np.median(moved) > 1e6 * np.median(bound_x)        # ... after having gone somewhere
        else:
            assert ir.frac("reversed x (f64)", x, c.x[:n].astype(LD), bound_x) <= 1.0
            assert ir.frac("reversed v (f64)", -v, c.v[:n].astype(LD), bound_v) <= 1.0


@pytest.mark.parametrize("n", ir.SIZES)
def test_the_nve_restatements_agree_at_every_size(n):
    c = ir.nve_case(n)
    L, F = _both(c)
    xl, vl = L.initial(c.x[:n], c.v[:n], c.f[:n], None)
    xf, vf = F.initial(c.x[:n], c.v[:n], c.f[:n], None)
    vl, ol = L.final(vl, c.f[:n])
    vf, of = F.final(vf, c.f[:n])
    val, mag = ir.out_arrays(ol)
    assert xf.shape == vf.shape == (n, 3) and xf.dtype == vf.dtype == np.float64
    assert max(ir.frac("x", xf, xl.v, ir.TOL * xl.m), ir.frac("v", vf, vl.v, ir.TOL * vl.m),
               ir.frac("d_out", np.array(of, dtype=np.float64), val, ir.TOL * mag)) <= 1.0
    assert not val[:, 2:].any()


def test_at_the_target_with_a_zero_chain_the_first_factor_is_one():
    c = ir.nvt_two()
    n = c.nlocal
    for kind in ("ld", "f64"):
        R = ir.Rule(kind, c)
        t0 = [tc for _, tc in ir.Rule("f64", c).temp(c.v[:n])]                 # the float64 temperatures: the targets
        R.setup(c.v[:n], t0)
        for g in range(2):
            R.S[g].t_target = R.num(t0[g])
            factor = R.chain_half_step(g)
            assert np.float64(factor.v if kind == "ld" else factor) == 1.0


def test_the_cases_contain_what_the_gpu_tests_claim():
    assert ir.SIZES == (1, 63, 64, 65, 255, 256, 257, 1000, 4097)
    for n in ir.SIZES + (ir.BIG,):
        c = ir.nve_case(n)
        assert c.nlocal == n and len(c.group) == n and c.x.shape == c.v.shape == c.f.shape == (n + ir.SENTINELS, 3)
        assert not c.style.any() and set(c.group) <= {-1, 0, 1}
        if n >= 8:
            assert (c.group == -1).any() and (c.group >= 0).any()
        assert np.all(c.type[c.group == -1] == 5) and c.type.min() >= 1 and c.type.max() <= len(c.mass)
    for edge in (ir.BLOCK - 1, ir.BLOCK, ir.BLOCK + 1, 63, 64, 65):
        assert edge in ir.SIZES
    assert ir.BIG > ir.BLOCK * ir.FINISH                                          # more rows of partial sums than finishing threads
    one, two, eight, big = ir.nvt_cases()
    assert [len(c.style) for c in (one, two, eight, big)] == [1, 2, 8, 2] and all(c.style.all() for c in (one, two, eight, big))
    assert big.nlocal == ir.BIG and eight.nlocal == 4097
    for c in (two, eight, big):                                                   # interleaved ids: every populated group in every quarter
        q = c.nlocal // 4
        big_groups = [g for g in range(len(c.style)) if c.count[g] > 100]
        assert len(big_groups) >= 2
        assert all(all((c.group[k * q:(k + 1) * q] == g).any() for k in range(4)) for g in big_groups)
    assert eight.count[3] == 1 and eight.count[5] == 0
    rows6 = np.nonzero(eight.group == 6)[0]
    assert len(rows6) == 40 and rows6.min() >= ir.BLOCK and rows6.max() < 2 * ir.BLOCK
    assert np.all(eight.dof > 0) and eight.dof[3] == 3.0 and eight.dof[0] == 3.0 * eight.count[0] - 3.0
    m = ir.mixed()
    assert list(m.style) == [0, 1] and (m.group == 0).any() and (m.group == 1).any()
    assert list(ir.as_nve(m).style) == [0, 0] and ir.as_nve(m).group is m.group
    # the seeded states are mid-run states: nothing in them is zero
    assert all(np.all(c.state0 != 0) for c in (one, two, eight, big))
