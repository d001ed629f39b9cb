"""no GPU: the reference of tests/dihedral_ref.py against itself, for all four styles -- forces as the derivative of its energy, forces
and torques that sum to zero, the virial in absolute coordinates, the convention of phi, the opls energies at phi = 0, pi / 2 and
pi -- and the float64 restatement of the kernels' arithmetic within a tenth of the GPU tests' bound on every input those tests use."""
import os
import re

import numpy as np
import pytest

import dihedral_ref as dr

LD = np.longdouble
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lammps-user-conp2_amd", "csrc")
PAIR_NAMES = ["opls", "cos"]


def test_launch_shapes_restated():
    """dihedral_ref restates the launch shapes of conp_dihedral.hip: whoever changes one there is sent here"""
    k = open(os.path.join(CSRC, "conp_kernels.h")).read()
    val = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", k).group(1))
    assert (val("DIHEDRAL_BLOCK"), val("DIHEDRAL_FINISH"), val("DIHEDRAL_TERM_W")) == (dr.BLOCK, dr.FINISH, dr.TERM_W)
    src = open(os.path.join(CSRC, "conp_dihedral.hip")).read()
    assert "r += DIHEDRAL_FINISH" in src and "blockIdx.x * DIHEDRAL_BLOCK + threadIdx.x" in src
    assert "atomic" not in src.split("#include", 1)[1] and "asm" not in src


def _energy_of(c, R):
    """E(y) of the case in longdouble on positions y [nall][3], the images of the reference held fixed while an atom moves"""
    t, prd = R.terms, np.asarray(c.prd, dtype=LD)
    s1, s3, s4 = R.geom.s1 * prd, R.geom.s3 * prd, R.geom.s4 * prd

    def energy(y):
        T = dr.terms_of(LD, y[t[:, 0]] + s1, y[t[:, 1]], y[t[:, 2]] + s3, y[t[:, 3]] + s4, R.form, R.k)
        return T.e.sum()
    return energy


def _central_difference(c, R, h, coords):
    energy = _energy_of(c, R)
    x = c.x.astype(LD)
    out = []
    for i, d in coords:
        yp, ym = x.copy(), x.copy()
        yp[i, d] += h; ym[i, d] -= h
        out.append(-(energy(yp) - energy(ym)) / (2 * h))
    return np.array(out, dtype=LD)


@pytest.mark.parametrize("pair", PAIR_NAMES)
def test_forces_are_minus_the_gradient_of_the_energy(pair):
    """longdouble central differences with step h = 1e-5 A, to 1e-8 of A.  What longdouble allows: the quotient's truncation is
    h^2 / 6 of the third derivative, (n / lever arm)^2 = (4 / 0.45 A)^2 = 80 / A^2 of the force at most, 1.3e-9 of it; its rounding
    is 1.1e-19 of the energy (some 100) over h, 1e-12 absolute.  Closest images through every face"""
    c = dr.molecules(pair, True, "image")
    R = dr.for_case(c)
    sh = np.concatenate([R.geom.s1, R.geom.s3, R.geom.s4])
    assert {-1, 1} <= set(sh[:, 0]) and {-1, 1} <= set(sh[:, 1])
    assert dr.conditioning(R) >= 0.5 - 1e-9
    # (the quadratic improper has a kink at phi = 0 and at |phi| = pi: no term sits on one)
    assert np.abs(R.T.phi).min() > 1e-3 and (np.pi - np.abs(R.T.phi)).min() > 1e-3
    used = np.unique(R.terms[:, :4].reshape(-1))
    coords = [(i, d) for i in used for d in range(3)]
    g = _central_difference(c, R, LD(1e-5), coords)
    want = np.array([R.f[i, d] for i, d in coords])
    bound = np.array([R.A[i, d] for i, d in coords])
    worst = float((np.abs(g - want) / (1e-8 * bound)).max())
    print(f"{pair}: -dE/dx against f: {worst:.3g} of 1e-8 A")
    assert worst <= 1.0
    untouched = np.setdiff1d(np.arange(c.nall), used)
    assert len(untouched) > 1 and np.all(R.f[untouched] == 0) and np.all(R.A[untouched] == 0)


def test_the_difference_quotient_of_the_device_only_check():
    """h = 1e-4 A: the reference's own quotient stays within a tenth of the GPU check's bound, 1e-5 of the largest force component
    (truncation h^2 / 6 * 80 / A^2 = 1.3e-7 of a force; a float64 energy of some 100 rounds to 1e-14, 5e-11 over 2 h)"""
    c = dr.difference_case()
    R = dr.for_case(c)
    assert len(c.impropers) == 0 and R.eng[1] == 0
    used = np.unique(R.terms[:, :4].reshape(-1))
    coords = [(i, d) for i in used for d in range(3)]
    g = _central_difference(c, R, LD(dr.DIFF_H), coords)
    want = np.array([R.f[i, d] for i, d in coords])
    worst = float(np.abs(g - want).max() / (0.1 * dr.DIFF_BOUND * np.abs(R.f).max()))
    print(f"difference quotient at h = {dr.DIFF_H:g}: {worst:.3g} of a tenth of the bound")
    assert worst <= 1.0


@pytest.mark.parametrize("pair", PAIR_NAMES)
def test_forces_and_torques_sum_to_zero(pair):
    """per term, about member 2, in longdouble: to 1e-16 of the sum of |lever| |f|_abs"""
    R = dr.for_case(dr.molecules(pair, True, "image"))
    T = R.T
    assert np.all(T.f1 + T.f2 + T.f3 + T.f4 == 0) or np.abs((T.f1 + T.f2 + T.f3 + T.f4)).max() <= 1e-18 * T.f2_abs.max()
    lev = [T.F, -T.G, T.H - T.G]
    tq = sum(np.cross(l, f) for l, f in zip(lev, (T.f1, T.f3, T.f4)))
    mag = sum(np.abs(l).sum(axis=1)[:, None] * fa.sum(axis=1)[:, None] for l, fa in zip(lev, (T.f1_abs, T.f3_abs, T.f4_abs)))
    assert np.all(np.abs(tq) <= 1e-16 * mag)
    assert np.all(np.abs(R.f.sum(axis=0)) <= 1e-17 * R.A.sum(axis=0))


@pytest.mark.parametrize("pair", PAIR_NAMES)
def test_the_virial_is_the_sum_of_x_f_in_absolute_coordinates(pair):
    """with prd = 0 (the ghost-index form): W = sum over atoms of x_i (x) f_i, and the per-atom sums are the totals"""
    c = dr.molecules(pair, True, "ghost")
    assert c.prd == (0.0, 0.0, 0.0)
    R = dr.for_case(c)
    x = c.x.astype(LD)
    W = dr._six(x, R.f).sum(axis=0)
    mag = dr._six(np.abs(x), R.A).sum(axis=0)
    assert np.all(np.abs(W - R.W) <= 1e-16 * mag)
    assert abs(R.eatom.sum() - R.eng.sum()) <= 1e-17 * R.E_abs.sum()
    assert np.all(np.abs(R.vatom.sum(axis=0) - R.W) <= 1e-17 * R.W_abs)


def test_trans_is_pi_cis_is_zero_and_the_opls_energies():
    c = dr.exact("opls")
    R = dr.for_case(c)
    phi = R.T.phi
    pi = np.arctan2(LD(0), LD(-1))
    assert phi[0] == 0 and not np.signbit(phi[0]) and phi[1] == pi and abs(phi[2] - pi / 2) < 1e-18
    K = c.p.dcoef.astype(LD)
    e = R.T.e
    assert abs(e[0] - (K[0, 0] + K[0, 2])) <= 1e-18 * np.abs(K[0]).sum()                       # E(0) = K1 + K3
    assert abs(e[1]) <= 1e-18 * np.abs(K[2]).sum()                                             # E(pi) = 0
    assert abs(e[2] - LD(0.5) * (K[2, 0] + 2 * K[2, 1] + K[2, 2])) <= 1e-18 * np.abs(K[2]).sum()     # E(pi / 2) = (K1 + 2 K2 + K3) / 2
    # the impropers of the same members: K (|phi| - chi0)^2
    k, chi = c.p.icoef[0].astype(LD)
    assert abs(e[5] - k * chi * chi) <= 1e-18 * k and abs(e[6] - k * (phi[1] - chi) ** 2) <= 1e-17 * k * 10
    # collinear members and coinciding members: nothing at all
    for t in (3, 4, 7, 8):
        assert not R.T.ok[t] and R.T.e[t] == 0 and not R.T.f1[t].any() and not R.T.f2[t].any() and not R.T.v[t].any()
    assert np.all(R.f[6:14] == 0) and np.all(R.A[6:14] == 0) and np.all(R.f[14] == 0)
    # the cosine styles on the same geometry: K (1 + d cos(n phi))
    c2 = dr.exact("cos")
    R2 = dr.for_case(c2)
    K, d, n = c2.p.dcoef[0].astype(LD)
    assert abs(R2.T.e[0] - K * (1 + d)) <= 1e-18 * K
    K, d, n = c2.p.dcoef[2].astype(LD)
    assert abs(R2.T.e[1] - K * (1 + d * np.cos(n * phi[1]))) <= 1e-18 * K


@pytest.mark.parametrize("pair", PAIR_NAMES)
def test_the_closest_image_form_is_the_ghost_index_form(pair):
    ci, cg = dr.molecules(pair, True, "image"), dr.molecules(pair, True, "ghost")
    Ri, Rg = dr.for_case(ci), dr.for_case(cg)
    nd, ni = len(ci.dihedrals), len(ci.impropers)
    sel = np.r_[0:nd, nd + 1:nd + 1 + ni]                # (the ghost form carries one dihedral and one improper more)
    for name in ("p1", "p3", "p4"):
        assert getattr(Rg.geom, name)[sel].tobytes() == getattr(Ri.geom, name).tobytes()
    for name in ("e", "f1", "f3", "f4", "v"):            # (longdouble: compared by value, its padding bytes are not data)
        assert np.array_equal(getattr(Rg.T, name)[sel], getattr(Ri.T, name))
    Rg2 = dr.reference(cg.x, cg.nlocal, cg.dihedrals[:nd], cg.impropers[:ni], cg.p, True)
    assert np.any(Rg2.f[cg.nlocal:] != 0)
    ff, fa = dr.fold(Rg2.f, cg.owner, cg.nlocal), dr.fold(Rg2.A, cg.owner, cg.nlocal)
    assert np.all(np.abs(ff - Ri.f) <= 1e-17 * fa) and np.all(np.abs(fa - Ri.A) <= 1e-17 * fa)


def test_the_inputs_have_what_the_kernels_can_go_wrong_on():
    s, dihedrals, impropers = dr.molecule_system()
    assert len(dihedrals) == 15 and len(impropers) == 15 and len(set(dihedrals[:, 4])) == 3 and len(set(impropers[:, 4])) == 2
    used = np.unique(dihedrals[:, :4].reshape(-1))
    assert np.sum(s.echeck[used] != 0) == 0 and np.sum(s.echeck == 0) == len(used) + 4
    # both style pairs carry every style's special rows: a chi0 that is not 0 and one that is; n = 0 and n = 3; d = +1 and d = -1
    assert set(dr.PARAMS_OPLS.icoef[:, 1] != 0) == {True, False}
    assert {0.0, 3.0} <= set(dr.PARAMS_COS.dcoef[:, 2]) and set(dr.PARAMS_COS.dcoef[:, 1]) == {1.0, -1.0} == set(dr.PARAMS_COS.icoef[:, 1])
    # closest-image form: s = +1 and s = -1 occur in x and in y, and one term is shifted in two dimensions (an edge)
    Ri = dr.for_case(dr.molecules("opls", True, "image"))
    sh = np.concatenate([Ri.geom.s1, Ri.geom.s3, Ri.geom.s4])
    assert {-1, 1} <= set(sh[:, 0]) and {-1, 1} <= set(sh[:, 1])
    assert np.any((sh[:, 0] != 0) & (sh[:, 1] != 0))
    # ghost-index form, newton off: terms with 0, 1, 2, 3 and 4 owned members
    cg = dr.molecules("opls", False, "ghost")
    owned = (np.concatenate([cg.dihedrals, cg.impropers])[:, :4] < cg.nlocal).sum(axis=1)
    assert {0, 4} <= set(owned) and len(set(owned) & {1, 2, 3}) >= 2, set(owned)
    R = dr.for_case(cg)
    assert np.all(R.f[cg.nlocal:] == 0) and np.all(R.eatom[cg.nlocal:] == 0)
    # hub: more slots than a wavefront has lanes, a ragged tail, every role
    h = dr.hub()
    t = np.concatenate([h.dihedrals, h.impropers])
    slots = np.bincount(t[:, :4].reshape(-1), minlength=h.nall)
    assert slots[0] == 70 and slots[0] % 64 != 0 and np.sum(slots == 0) == 2
    assert all((t[:, r] == 0).sum() >= 17 for r in range(4))
    assert all((h.dihedrals[:, r] == 0).any() and (h.impropers[:, r] == 0).any() for r in range(4))
    # edges: the shapes, the last atom in a term, and with newton off some members are ghosts
    B = dr.BLOCK
    assert {(a, b) for a, b, n, _ in dr.EDGE_SHAPES if n is None and a * b == 0} == {(B - 1, 0), (B, 0), (B + 1, 0), (0, B - 1), (0, B), (0, B + 1)}
    assert {a + b for a, b, n, _ in dr.EDGE_SHAPES if a * b != 0 and a < B} >= {B - 1, B, B + 1}
    assert {n for a, b, n, _ in dr.EDGE_SHAPES if n is not None} == {B - 1, B + 1}
    for shape in dr.EDGE_SHAPES[:-1]:
        e = dr.edge_case(shape)
        assert (len(e.dihedrals), len(e.impropers)) == shape[:2] and (shape[2] is None or e.nall == shape[2])
        assert e.nall - 1 in np.concatenate([e.dihedrals, e.impropers])[:, :4]
    e = dr.edge_case((129, 128, None, "cos"), newton=False)
    assert len(set((e.dihedrals[:, :4] < e.nlocal).sum(axis=1))) >= 2


def test_the_float64_restatement_stays_within_a_tenth_of_the_bound_on_every_gpu_input():
    """the condition the GPU bound rests on: bond-angle sines of 0.25 or more, and then float64 in the kernels' order is within
    TOL / 10 of the magnitudes"""
    worst = 0.0
    for c in dr.gpu_cases():
        R = dr.for_case(c)
        assert dr.conditioning(R) >= 0.25, c.tag
        got = dr.restate64(c.x, c.nlocal, c.dihedrals, c.impropers, c.p, c.newton, c.prd)
        fr = dr.check(c.tag + " (float64 restatement)", got, R, tol=dr.TOL / 10)
        worst = max(worst, max(fr.values()))
    print(f"float64 restatement: at most {worst:.3g} of a tenth of the bound")
