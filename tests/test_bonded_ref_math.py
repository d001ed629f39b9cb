"""no GPU: the reference of tests/bonded_ref.py against itself -- forces as the derivative of its energy, the per-atom identities, the
closest-image form against the ghost-index form -- and the float64 restatement of the kernels' arithmetic within the GPU tests'
bound on every input those tests use."""
import os
import re

import numpy as np
import pytest

import bonded_ref as br

LD = np.longdouble
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "lammps-user-conp2_amd", "csrc")


def test_launch_shapes_restated():
    """bonded_ref restates the launch shapes of conp_bonded.hip: whoever changes one there is sent here"""
    k = open(os.path.join(CSRC, "conp_kernels.h")).read()
    val = lambda name: int(re.search(rf"constexpr int {name} = (\d+);", k).group(1))
    assert (val("BONDED_BLOCK"), val("BONDED_FINISH"), val("BONDED_TERM_W")) == (br.BLOCK, br.FINISH, br.TERM_W)
    src = open(os.path.join(CSRC, "conp_bonded.hip")).read()
    assert "r += BONDED_FINISH" in src and "blockIdx.x * BONDED_BLOCK + threadIdx.x" in src


def test_forces_are_minus_the_gradient_of_the_energy():
    """longdouble central differences with step 1e-6 A, to 1e-8 of A; angles between 30 and 150 degrees, closest images through
    every face"""
    c = br.molecules(True, "image")
    R = br.for_case(c)
    assert all({-1, 1} <= set(np.concatenate([R.geom.sb[:, d], R.geom.s1[:, d], R.geom.s3[:, d]])) for d in range(3))
    ang = np.degrees(np.arccos(R.geom.c))
    assert ang.min() >= 30.0 - 1e-9 and ang.max() <= 150.0 + 1e-9
    h = LD(1e-6)
    x = c.x.astype(LD)
    # the images of the reference stay fixed while an atom moves by h: the energy is evaluated on unwrapped partner coordinates
    b, a = R.bonds, R.angles
    prd = np.asarray(c.prd, dtype=LD)
    sb, s1, s3 = R.geom.sb * prd, R.geom.s1 * prd, R.geom.s3 * prd
    p = c.p
    bk, b0 = np.concatenate([[0], p.bond_k]).astype(LD)[b[:, 2]], np.concatenate([[0], p.bond_r0]).astype(LD)[b[:, 2]]
    ak, a0 = np.concatenate([[0], p.angle_k]).astype(LD)[a[:, 3]], np.concatenate([[0], p.angle_theta0]).astype(LD)[a[:, 3]]

    def energy(y):
        d = y[b[:, 0]] - (y[b[:, 1]] + sb)
        e = (bk * (np.sqrt((d * d).sum(axis=1)) - b0) ** 2).sum()
        d1, d2 = y[a[:, 0]] + s1 - y[a[:, 1]], y[a[:, 2]] + s3 - y[a[:, 1]]
        cc = (d1 * d2).sum(axis=1) / np.sqrt((d1 * d1).sum(axis=1) * (d2 * d2).sum(axis=1))
        return e + (ak * (np.arccos(cc) - a0) ** 2).sum()
    used = np.unique(np.concatenate([b[:, :2].reshape(-1), a[:, :3].reshape(-1)]))
    worst = 0.0
    for i in used:
        for d in range(3):
            yp, ym = x.copy(), x.copy()
            yp[i, d] += h; ym[i, d] -= h
            g = -(energy(yp) - energy(ym)) / (2 * h)
            worst = max(worst, float(abs(g - R.f[i, d]) / (1e-8 * R.A[i, d])))
    print(f"-dE/dx against f: {worst:.3g} of 1e-8 A")
    assert worst <= 1.0
    untouched = np.setdiff1d(np.arange(c.nall), used)
    assert len(untouched) > 1 and np.all(R.f[untouched] == 0) and np.all(R.A[untouched] == 0)


@pytest.mark.parametrize("form", ["image", "ghost"])
def test_per_atom_sums_are_the_totals_with_newton(form):
    R = br.for_case(br.molecules(True, form))
    assert abs(R.eatom.sum() - R.eng.sum()) <= 1e-17 * R.E_abs.sum()
    assert np.all(np.abs(R.vatom.sum(axis=0) - R.W) <= 1e-17 * R.W_abs)


def test_the_closest_image_form_is_the_ghost_index_form():
    ci, cg = br.molecules(True, "image"), br.molecules(True, "ghost")
    Ri, Rg = br.for_case(ci), br.for_case(cg)
    nb, na = len(ci.bonds), len(ci.angles)
    # the ghost coordinates are the images, bit for bit, and so are the terms (the ghost form carries one bond and angle more)
    assert Rg.geom.bx2[:nb].tobytes() == Ri.geom.bx2.tobytes() and Rg.geom.a1[:na].tobytes() == Ri.geom.a1.tobytes()
    assert Rg.geom.a3[:na].tobytes() == Ri.geom.a3.tobytes()
    for name in ("e", "f1", "v"):                        # (longdouble: compared by value, its padding bytes are not data)
        assert np.array_equal(getattr(Rg.B, name)[:nb], getattr(Ri.B, name))
    for name in ("e", "f1", "f3", "v"):
        assert np.array_equal(getattr(Rg.Ang, name)[:na], getattr(Ri.Ang, name))
    # without the ghost-only terms the folded forces are the closest-image forces
    Rg2 = br.reference(cg.x, cg.nlocal, cg.bonds[:nb], cg.angles[:na], cg.p, True)
    assert np.any(Rg2.f[cg.nlocal:] != 0)
    ff, fa = br.fold(Rg2.f, cg.owner, cg.nlocal), br.fold(Rg2.A, cg.owner, cg.nlocal)
    assert np.all(np.abs(ff - Ri.f) <= 1e-17 * fa)
    assert np.all(Ri.f[ci.nlocal:] == 0) and np.all(np.abs(fa - Ri.A) <= 1e-17 * fa)


def test_the_inputs_have_what_the_kernels_can_go_wrong_on():
    s, bonds, angles = br.molecule_system()
    assert len(bonds) == 42 and len(angles) == 21 and len(set(bonds[:, 2])) == 3 and len(set(angles[:, 3])) == 2
    used = np.unique(np.concatenate([bonds[:, :2].reshape(-1), angles[:, :3].reshape(-1)]))
    assert np.sum(s.echeck[used] != 0) == 0 and np.sum(s.echeck == 0) == len(used) + 1
    # closest-image form: s = +1 and s = -1 occur in x and in y, and one term is shifted in two dimensions (an edge)
    Ri = br.for_case(br.molecules(True, "image"))
    sh = np.concatenate([Ri.geom.sb, Ri.geom.s1, Ri.geom.s3])
    assert {-1, 1} <= set(sh[:, 0]) and {-1, 1} <= set(sh[:, 1])
    assert np.any((sh[:, 0] != 0) & (sh[:, 1] != 0))
    # ghost-index form: molecules straddle each periodic face and one edge, seen from the ghosts' shifts
    cg = br.molecules(False, "ghost")
    prd = np.where(s.periodic, s.prd, 1.0)
    gs = np.rint((cg.x - cg.x[cg.owner]) / prd).astype(int)
    members = np.concatenate([cg.bonds[:, :2].reshape(-1), cg.angles[:, :3].reshape(-1)])
    msh = gs[members]
    for d in range(3):
        if s.periodic[d]:
            assert {-1, 1} <= set(msh[:, d]), d
    assert np.any((msh[:, 0] != 0) & (msh[:, 1] != 0))
    # newton off: terms with 1 of 2, 1 of 3, 2 of 3 owned members and one with none
    ob = (cg.bonds[:, :2] < cg.nlocal).sum(axis=1)
    oa = (cg.angles[:, :3] < cg.nlocal).sum(axis=1)
    assert {0, 1, 2} <= set(ob) and {0, 1, 2, 3} <= set(oa)
    R = br.for_case(cg)
    assert np.all(R.f[cg.nlocal:] == 0) and np.all(R.eatom[cg.nlocal:] == 0)
    # hub: more slots than a wavefront has lanes, a ragged tail
    h = br.hub()
    slots = np.bincount(np.concatenate([h.bonds[:, :2].reshape(-1), h.angles[:, :3].reshape(-1)]), minlength=h.nall)
    assert slots[0] == 140 and slots[0] > 2 * 64 and slots[0] % 64 != 0 and np.sum(slots == 0) == 2
    # degenerate terms
    D = br.for_case(br.degenerate())
    assert D.geom.r[0] == 0.0 and np.all(D.B.f1[0] == 0) and D.B.e[0] == LD(br.PARAMS.bond_k[0]) * LD(br.PARAMS.bond_r0[0]) ** 2
    assert D.geom.c[0] == -1.0 and D.geom.c[1] == 1.0
    assert abs(np.degrees(np.arccos(D.geom.c[2])) - 179.97) < 1e-6 and 4e-4 < np.sqrt(1 - D.geom.c[2] ** 2) < 1e-3
    assert 0 < abs(D.geom.r[1] - br.PARAMS.bond_r0[1]) < 1e-9
    assert 0 < abs(np.arccos(D.geom.c[3]) - br.PARAMS.angle_theta0[0]) < 1e-9
    assert np.all(np.isfinite(D.f.astype(float))) and np.all(D.f[16] == 0)
    # edges: the last atom is in a term, and with newton off some members are ghosts
    for shape in br.EDGE_SHAPES:
        e = br.edges(*shape)
        assert (len(e.bonds), len(e.angles)) == shape[:2] and (shape[2] is None or e.nall == shape[2])
        assert e.nall - 1 in np.concatenate([e.bonds[:, :2].reshape(-1), e.angles[:, :3].reshape(-1)])
    e = br.edges(172, 85, 2 * br.BLOCK + 1, newton=False)
    assert {0, 1, 2} & set((e.bonds[:, :2] < e.nlocal).sum(axis=1)) >= {1, 2}


def test_the_float64_restatement_stays_within_the_bound_on_every_gpu_input():
    for c in br.gpu_cases():
        R = br.for_case(c)
        assert br.conditioning(R) >= 2e-4, c.tag            # the condition under which an ulp of c stays inside the bound
        got = br.restate64(c.x, c.nlocal, c.bonds, c.angles, c.p, c.newton, c.prd)
        br.check(c.tag + " (float64 restatement)", got, R)
