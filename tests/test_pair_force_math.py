"""No GPU, no library: the numpy reference of tests/pair_force_ref.py against its own energy, its own sums, a brute-force sum and
the analytic effect of the special-bond factors -- before it judges the library (tests/test_gpu_pair_*.py)."""
import dataclasses
import functools

import numpy as np
import pytest
from scipy.special import erfc as erfc_exact

import pair_force_ref as pref
from conp_amd import neighbor, systems

LD = np.longdouble
QS = systems.QQRD2E


@functools.lru_cache(maxsize=None)
def _case(newton, special_frac=0.0, cutoff=8.0):
    s = dataclasses.replace(systems.small_random(ne_side=4, n_elyte=64, seed=pref.SEED, cutoff=cutoff), newton=newton, eletypes=None)
    at, lst, _ = neighbor.build_lists(s, special_frac=special_frac)
    return s, at, lst, pref.lj_tables(s.ntypes, s.cutoff)


def _with_ghosts(at, x_owned):
    """all positions when the owned atoms sit at x_owned and every ghost keeps its shift to its owner"""
    shift = at.x - at.x[at.owner]
    return x_owned[at.owner] + shift


@pytest.mark.parametrize("newton", [False, True])
def test_forces_are_the_gradient_of_the_energy(newton):
    s, at, lst, p = _case(newton)
    n, h = at.nlocal, 1e-4
    R = pref.for_atoms(at, lst, p, s, newton)
    f = pref.fold(R.f, at.owner, n) if newton else R.f[:n]
    if not newton:
        assert np.all(R.f[n:] == 0)                       # ghost rows are not touched
    # atoms none of whose pairs comes within 2 h of a cutoff (cut_coul = the pair cutoff, and the three LJ cutoffs): the energy
    # of the pair style jumps there (the Coulomb part is not shifted), and a central difference must not straddle a jump
    cuts = np.unique(np.concatenate([[s.cutoff], np.sqrt(p.lj["cut_ljsq"]).ravel()]))
    i, jraw = pref.pairs_of(lst)
    j = jraw & pref.NEIGHMASK
    r = np.sqrt(((at.x[i] - at.x[j]) ** 2).sum(axis=1))
    near = np.abs(r[:, None] - cuts[None, :]).min(axis=1) < 4 * h
    dirty = np.zeros(n, bool)
    dirty[at.owner[i[near]]] = True
    dirty[at.owner[j[near]]] = True
    charged = np.nonzero(~dirty & (at.q[:n] != 0))[0][:4]
    neutral = np.nonzero(~dirty & (at.q[:n] == 0))[0][:2]
    pick = np.concatenate([charged, neutral])
    assert len(charged) == 4 and len(neutral) == 2 and not dirty[pick].any()

    def energy(x_owned):
        return pref.for_atoms(at, lst, p, s, newton, x=_with_ghosts(at, x_owned)).eng.sum()
    x0 = np.asarray(at.x[:n], dtype=LD)
    fd = np.zeros((len(pick), 3), dtype=LD)
    for k, a in enumerate(pick):
        for c in range(3):
            xp, xm = x0.copy(), x0.copy()
            xp[a, c] += LD(h); xm[a, c] -= LD(h)
            fd[k, c] = -(energy(xp) - energy(xm)) / (2 * LD(h))
    # Tolerance, per atom.  (a) h^2 f''' / 6: the steepest term is r^-13 (f''' = 14 * 15 / r^2 f), at the smallest distance 0.8 A
    # 1e-8 / 6 * 210 / 0.64 = 5.5e-7 of the force magnitude A_i; 1e-6 A_i leaves room.  (b) The force is the derivative of the EXACT
    # erfc (pair_lj_cut_coul_long.cpp), the energy uses the polynomial: they differ by |pre| g |d/dx (poly - erfc)|, at most D per unit
    # of sum |pre| g, D evaluated here on a grid.  Rounding of E in longdouble: 1e-19 E_abs / h, nothing.
    xs = np.linspace(0.0, s.g_ewald * s.cutoff, 20001)
    delta = np.asarray(pref.erfc_poly(xs.astype(LD), np.exp(-(xs.astype(LD)) ** 2)), dtype=float) - erfc_exact(xs)
    D = np.abs(np.gradient(delta, xs)).max()
    assert 1e-7 < D < 1e-5, D
    pre_sum = np.zeros(at.nall)
    np.add.at(pre_sum, R.i, np.abs(R.terms.pre.astype(float)))
    np.add.at(pre_sum, R.j, np.abs(R.terms.pre.astype(float)))
    pre_own = pref.fold(pre_sum, at.owner, n)
    A_own = pref.fold(R.A.astype(float), at.owner, n)
    tol = 1e-6 * A_own[pick] + 1.5 * D * s.g_ewald * pre_own[pick]
    err = np.abs((f[pick] - fd).astype(float)).max(axis=1)
    print("finite differences: error / tolerance per atom", err / tol, " D =", D)
    assert np.all(err <= tol), (err, tol)                 # observed: at most 0.05 of the tolerance
    assert np.abs(fd[:4]).max() > 1.0 and np.abs(fd[4:]).max() > 0.1     # real forces, also on the zero-charge atoms (LJ)


@pytest.mark.parametrize("newton", [False, True])
@pytest.mark.parametrize("special", [False, True])
def test_per_atom_sums_equal_the_totals(newton, special):
    s, at, lst, p = _case(newton, 0.2 if special else 0.0)
    R = pref.for_atoms(at, lst, p, s, newton, *((pref.SPECIAL_LJ, pref.SPECIAL_COUL) if special else ()))
    assert abs(R.eatom.sum() - R.eng.sum()) <= 1e-13 * R.E_abs
    assert np.all(np.abs(R.vatom.sum(axis=0) - R.W) <= 1e-13 * R.W_abs)
    assert R.E_abs > 0 and np.all(R.W_abs > 0)
    if not newton:
        assert np.all(R.eatom[at.nlocal:] == 0) and np.all(R.vatom[at.nlocal:] == 0)


def test_newton_on_and_off_agree():
    s0, at0, l0, p = _case(False)
    s1, at1, l1, _ = _case(True)
    assert l1.npairs < l0.npairs and at0.nall == at1.nall
    R0, R1 = pref.for_atoms(at0, l0, p, s0, False), pref.for_atoms(at1, l1, p, s1, True)
    n = at0.nlocal
    assert abs(R0.eng[0] - R1.eng[0]) <= 1e-13 * R0.E_abs and abs(R0.eng[1] - R1.eng[1]) <= 1e-13 * R0.E_abs
    assert np.all(np.abs(R0.W - R1.W) <= 1e-13 * R0.W_abs)
    f1, A = pref.fold(R1.f, at1.owner, n), pref.fold(R0.A, at0.owner, n)
    assert np.all(np.abs(R0.f[:n] - f1) <= 1e-13 * A[:, None])
    assert np.all(np.abs(R0.eatom[:n] - pref.fold(R1.eatom, at1.owner, n)) <= 1e-13 * R0.E_abs)


@pytest.mark.parametrize("newton", [False, True])
def test_half_list_equals_the_brute_force_sum_over_minimum_images(newton):
    s, at, lst, p = _case(newton, cutoff=4.0)
    prd = np.asarray(s.prd)
    assert np.all(prd > 2 * s.cutoff)                     # one image per pair at most
    n = at.nlocal
    R = pref.for_atoms(at, lst, p, s, newton)
    a, b = np.triu_indices(n, 1)
    # one "list" of all owned pairs at their minimum-image separation: atom b is replaced by its nearest image, pair by pair
    x = np.asarray(at.x[:n], dtype=LD)
    d = x[a] - x[b]
    d -= np.asarray(prd, dtype=LD) * np.round((d / np.asarray(prd, dtype=LD)).astype(float))
    xa, xb = x[a], x[a] - d
    xs = np.concatenate([xa, xb])
    m = len(a)
    lst2 = neighbor.NeighList(inum=m, ilist=np.arange(m, dtype=np.int32), numneigh=np.concatenate([np.ones(m), np.zeros(m)]).astype(np.int32),
                              first=np.concatenate([np.arange(m), np.zeros(m)]).astype(np.int32), neigh=(m + np.arange(m)).astype(np.int32))
    typ2, q2 = np.concatenate([at.type[a], at.type[b]]), np.concatenate([at.q[a], at.q[b]])
    B = pref.reference(xs, q2, typ2, 2 * m, lst2, p, s.g_ewald, QS, True)
    fb = np.zeros((n, 3), dtype=LD)
    np.add.at(fb, a, B.f[:m]); np.add.at(fb, b, B.f[m:])
    f = pref.fold(R.f, at.owner, n) if newton else R.f[:n]
    A = pref.fold(R.A, at.owner, n)
    if newton:
        assert B.npairs == R.npairs               # every pair within the cutoff is listed once
    assert abs(B.eng[0] - R.eng[0]) <= 1e-13 * R.E_abs and abs(B.eng[1] - R.eng[1]) <= 1e-13 * R.E_abs
    assert np.all(np.abs(B.W - R.W) <= 1e-13 * R.W_abs)
    assert np.all(np.abs(fb - f) <= 1e-13 * A[:, None])
    assert R.E_abs > 0 and np.abs(f).max() > 0


def test_special_factors_change_the_result_by_the_expected_terms():
    s, at, lst, p = _case(False, 0.2)
    plain = pref.for_atoms(at, lst, p, s, False)                                  # bits stripped, every factor 1
    R = pref.for_atoms(at, lst, p, s, False, pref.SPECIAL_LJ, pref.SPECIAL_COUL)
    t, T = plain.terms, R.terms
    sb_marked = (T.fc < 1) | (T.fl < 1)
    assert 0.1 < sb_marked.mean() < 0.3 and {float(v) for v in np.unique(T.fc)} == {0.0, 0.5, 0.8333, 1.0}
    # energy: every marked pair loses (1 - fc) pre of its Coulomb energy and (1 - fl) of its LJ energy
    dE_coul = -(t.w * (1 - T.fc) * t.pre).sum()
    dE_lj = -(t.w * (1 - T.fl) * t.evdwl).sum()
    assert abs((R.eng[1] - plain.eng[1]) - dE_coul) <= 1e-13 * plain.E_abs
    assert abs((R.eng[0] - plain.eng[0]) - dE_lj) <= 1e-13 * plain.E_abs
    assert abs(dE_coul) > 1e-3 * np.abs(t.w * t.pre).sum() and abs(dE_lj) > 0
    # forces: fpair changes by -((1 - fc) pre + (1 - fl) forcelj) r2inv
    dfp = -((1 - T.fc) * t.pre + (1 - T.fl) * t.forcelj) * t.r2inv
    df = np.zeros_like(plain.f)
    np.add.at(df, plain.i[t.iw], (t.d * dfp[:, None])[t.iw])
    np.add.at(df, plain.j[t.jw], (-t.d * dfp[:, None])[t.jw])
    assert np.all(np.abs((R.f - plain.f) - df) <= 1e-13 * plain.A[:, None])
    # fc = 0: the pair's Coulomb energy is pre (erfc - 1), the real-space sum minus the bare 1 / r the bonded pair must not feel
    k = np.nonzero((T.fc == 0) & (np.abs(T.pre) > 0))[0][0]
    one = neighbor.NeighList(inum=1, ilist=np.array([0], np.int32), numneigh=np.array([1, 0], np.int32), first=np.array([0, 0], np.int32),
                             neigh=np.array([1 | (1 << 30)], np.int32))
    ij = [R.i[k], R.j[k]]
    P = pref.reference(at.x[ij], at.q[ij], at.type[ij], 2, one, pref.lj_tables(s.ntypes, s.cutoff, with_lj=False), s.g_ewald, QS, True,
                       pref.SPECIAL_LJ, pref.SPECIAL_COUL)
    x = LD(s.g_ewald) * R.r[k]
    assert abs(P.eng[1] - T.pre[k] * (pref.erfc_poly(x, np.exp(-x * x)) - 1)) <= 1e-15 * abs(T.pre[k])
    assert P.eng[0] == 0
