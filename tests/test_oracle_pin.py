"""Pins the CPU oracle to the only known-answer vector the reference's tests hold for this path:
tests/dilute/persist.log (G vector, step-0 electrode charges; ffield etypes, dV = 1 V)."""
import json
import os

import numpy as np
import pytest

from conp_amd import neighbor, systems
import oracle_py

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def run_oracle(lib, s, **kw):
    at, alist, blist = neighbor.build_lists(s)
    fx = oracle_py.Fix(lib, s, **kw)
    fx.set_atoms(at)
    fx.set_lists(alist, blist)
    fx.post_neighbor()
    info = fx.linalg_setup()
    assert info == 0
    fx.pre_force(s.potdiff)
    return fx, at


def test_dilute_step0_charge_matches_persist_log(oracle):
    gold = json.load(open(os.path.join(GOLD, "dilute_persist.json")))
    s = systems.deck("dilute", "ffield", etypes=True, g_ewald=gold["g_ewald"])
    fx, at = run_oracle(oracle, s)
    qleft = at.q[:at.nlocal][at.echeck[:at.nlocal] == 1].sum()
    qright = at.q[:at.nlocal][at.echeck[:at.nlocal] == -1].sum()
    step0 = gold["thermo"][0]
    print("oracle qleft", qleft, "persist.log", step0[3])
    # the log prints 8 significant digits
    assert qleft == pytest.approx(step0[3], rel=5e-7)
    assert qright == pytest.approx(step0[4], rel=5e-7)
    assert abs(qleft + qright) < 1e-14
    fx.close()


@pytest.mark.parametrize("mesh", [(12, 10, 18), (7, 11, 13)])
def test_fft_poisson_step_equals_the_plain_dft(oracle, mesh):
    """oracle_py.Pppm(fast=True) solves the oracle's brick with the oracle's influence function through numpy.fft (the reference of the
    production-sized PPPM tests): the same mesh potential as the plain per-axis DFT, on a smooth and on a non-smooth mesh, to 1e-13
    of the largest mesh value; through b_cal as well"""
    s = systems.deck("dilute", "ffield", etypes=True)
    rho = np.random.default_rng(1).normal(size=mesh[0] * mesh[1] * mesh[2])
    slow, fast = oracle_py.Pppm(oracle, s, mesh, 5), oracle_py.Pppm(oracle, s, mesh, 5, fast=True)
    (u0, i0), (u1, i1) = slow.poisson(mesh, rho), fast.poisson(mesh, rho)
    top = np.abs(u0).max()
    assert top > 0 and not np.array_equal(u0, u1)              # (two different routes)
    assert np.abs(u1 - u0).max() < 1e-13 * top and max(np.abs(i0).max(), np.abs(i1).max()) < 1e-13 * top
    at, _, _ = neighbor.build_lists(s)
    xele = at.x[:at.nlocal][at.echeck[:at.nlocal] != 0]
    b0, b1 = (p.b_cal(at.x, at.q, at.echeck, at.nlocal, xele) for p in (slow, fast))
    assert np.abs(b0).max() > 0 and np.abs(b1 - b0).max() < 1e-13 * np.abs(b0).max()
    slow.close(); fast.close()


@pytest.mark.parametrize("order", [4, 5])
def test_oracle_pppm_handles_atoms_outside_the_box(oracle, order):
    """atoms up to 1 A outside the periodic box and exactly on boxhi (helpers.push_outside): the oracle's index arithmetic is the
    reference's -- (int)(xs + shift) - OFFSET with xs < 0 or xs >= n, then the periodic wrap of every stencil point -- so the brick
    equals that of the wrapped positions, its total times the cell volume is the charge spread, and an atom on boxhi has mesh index n"""
    from helpers import push_outside, rel_err
    s = systems.deck("dilute", "ffield", etypes=True)
    mesh = (27, 24, 144)
    at, _, _ = neighbor.build_lists(s)
    moved = push_outside(s, at)
    n = at.nlocal
    pp = oracle_py.Pppm(oracle, s, mesh, order)
    _, _, out = pp.make_rho(mesh, at.x, at.q, at.echeck, n)
    for i in moved[12:]:                                        # on boxhi: xs = n, up to the rounding of the division
        c = int(np.nonzero(at.x[i] == s.boxhi)[0][0])
        xs = (at.x[i, c] - s.boxlo[c]) * (mesh[c] / s.prd[c])
        assert int(xs + (16384.5 if order % 2 else 16384.0)) - 16384 in (mesh[c] - 1, mesh[c])
    xw = at.x.copy()
    xw[:n] = s.boxlo + np.mod(at.x[:n] - s.boxlo, s.prd)
    assert np.all(xw[:n] >= s.boxlo) and np.all(xw[:n] < s.boxhi) and np.abs(xw[:n] - at.x[:n]).max() > 1.0
    _, _, wrapped = pp.make_rho(mesh, xw, at.q, at.echeck, n)
    assert np.abs(wrapped).max() > 0 and rel_err(out, wrapped) < 1e-10
    dv = (s.prd[0] / mesh[0]) * (s.prd[1] / mesh[1]) * (s.prd[2] / mesh[2])
    assert out.sum() * dv == pytest.approx(at.q[:n][at.echeck[:n] == 0].sum(), abs=1e-10)
    # the potentials read the mesh with the same arithmetic
    sel = np.zeros(n, np.int32); sel[moved] = 1
    u_out = pp.group_potential(at.x, at.q, at.echeck, n, sel)[moved]
    u_wr = pp.group_potential(xw, at.q, at.echeck, n, sel)[moved]
    assert np.abs(u_wr).max() > 0 and rel_err(u_out, u_wr) < 1e-10
    pp.close()
