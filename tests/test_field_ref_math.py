"""no GPU: the two restatements of tests/field_ref.py agree within the bound on every input of the GPU tests, and the rules satisfy
the identities that tie the field to the group sums: sum f = E qe2f sum q, energy = -(E . D) with D the dipole columns of the same
selection and images, trace of the virial = -energy, sum of the per-atom virial = the virial, and an atom moved by one box length with
its image counter decremented changes neither (beyond the bound), and the force not at all."""
import numpy as np
import pytest

import field_ref as fr
from field_ref import test_launch_shapes_restated  # noqa: F401  (collected here: field_ref.py itself is no test module)
from integrate_ref import LD, Mag

EFIELD_CASES = fr.efield_cases()
OBSERVE_CASES = fr.observe_cases()


def close(tag, a, b, n):
    """two Mag values that must agree: |a - b| within tol_of(n) of the sum of their magnitudes"""
    assert fr.frac(tag, a.v, b.v, fr.tol_of(n) * (a.m + b.m)) <= 1.0, tag


@pytest.mark.parametrize("k", range(len(EFIELD_CASES)))
def test_the_field_rule(k):
    c, e, opt = EFIELD_CASES[k]
    n = c.nlocal
    tag = f"{c.tag}, e {e}, {opt}"
    L, D = fr.efield("ld", c, e, **opt), fr.efield("f64", c, e, **opt)
    tol = fr.tol_of(n)
    # the two restatements
    assert fr.frac(f"{tag}: add", D.add, L.add.v, fr.TOL * L.add.m) <= 1.0
    assert fr.frac(f"{tag}: vatom", D.vatom, L.vatom.v, fr.TOL * L.vatom.m) <= 1.0
    assert fr.frac(f"{tag}: out", D.out[:10], L.out.v[:10], tol * L.out.m[:10]) <= 1.0
    assert D.out[10] == float(L.out.v[10]) == L.nsel == int((c.sel[:n] != 0).sum())
    unsel = c.sel[:n] == 0
    assert not D.vatom[unsel].any() and D.f[unsel].tobytes() == c.f[:n][unsel].tobytes()
    # against the group sums of the same selection and images
    O = fr.observe("ld", c, with_v=False, image=opt.get("image", True), mask=(c.sel != 0).astype(np.int32), ngroups=1)
    assert float(O.v[0, 0]) == L.nsel
    E = L.E
    for a in range(3):
        close(f"{tag}: sum f[{a}] = E qe2f sum q", L.out[1 + a], E[a] * O[0, 1], n)
    close(f"{tag}: energy = -(E . D)", L.out[0], -((E[0] * O[0, 2] + E[1] * O[0, 3]) + E[2] * O[0, 4]), n)
    close(f"{tag}: trace", (L.out[4] + L.out[5]) + L.out[6], -L.out[0], n)
    va = Mag(L.vatom.v.sum(axis=0), L.vatom.m.sum(axis=0))
    close(f"{tag}: sum vatom", va, L.out[4:10], n)
    # one box length further with the image counter decremented
    if opt.get("image", True):
        rows = np.arange(0, n, 3)
        x2, i2 = c.x.copy(), c.image.copy()
        x2[rows] += np.asarray(c.prd)
        i2[rows] -= 1
        L2, D2 = fr.efield("ld", c, e, x=x2, img=i2, **opt), fr.efield("f64", c, e, x=x2, img=i2, **opt)
        assert D2.f.tobytes() == D.f.tobytes() and D2.add.tobytes() == D.add.tobytes()
        bound = tol * (L.out.m[:10] + L2.out.m[:10])
        assert fr.frac(f"{tag}: moved, ld", L2.out.v[:10], L.out.v[:10], bound) <= 1.0
        assert fr.frac(f"{tag}: moved, f64", D2.out[:10], D.out[:10], bound) <= 1.0


@pytest.mark.parametrize("k", range(len(OBSERVE_CASES)))
def test_the_group_sums(k):
    c = OBSERVE_CASES[k]
    n = c.nlocal
    tol = fr.tol_of(n)
    for with_v in (True, False):
        for image in (True, False):
            L, D = fr.observe("ld", c, with_v, image), fr.observe("f64", c, with_v, image)
            assert D.shape == (c.ngroups, fr.OBSERVE_W)
            assert fr.frac(f"{c.tag}, v {with_v}, image {image}", D, L.v, tol * L.m) <= 1.0
            for g in range(c.ngroups):
                member = ((c.mask[:n] >> g) & 1) != 0
                assert D[g, 0] == member.sum()
                if not member.any():
                    assert not D[g].any()
            if not with_v:
                assert not D[:, 5:9].any()


def test_the_il_groups_nest_and_are_neutral():
    c = fr.il_case()
    D, L = fr.observe("f64", c), fr.observe("ld", c)
    sol, left, right, ele, all_ = (D[g] for g in range(5))
    # (il_onelayer: one layer of 416 atoms per electrode carries the fix; the other layers are in `ele` only)
    assert (sol[0], left[0], right[0], ele[0], all_[0]) == (1280, 416, 416, 2496, 3776)
    assert sol[0] + ele[0] == all_[0]
    assert abs(D[4, 1]) <= fr.tol_of(c.nlocal) * float(L.m[4, 1])
    assert D[3, 5] == 0.0                          # the electrodes do not move


def test_equal_masses_sum_to_n_m():
    c = fr.case("equal masses", 1000, seed=11, masks="nested")
    c = fr.with_(c, mass=np.full(5, 39.948))
    D, L = fr.observe("f64", c), fr.observe("ld", c)
    for g in range(c.ngroups):
        assert abs(LD(D[g, 9]) - LD(D[g, 0]) * LD(39.948)) <= fr.tol_of(c.nlocal) * L.m[g, 9]


def test_the_coupled_field():
    """ez = qe2f (e[2] + couple_scale s): at e[2] = 0 and couple_scale = -1 / lz the field the decks' `variable efi equal -f_e/lz` gives"""
    c = fr.case("coupled", 1000, seed=13)
    s, lz = 1.734, c.prd[2]
    L = fr.efield("ld", c, (0.0, 0.0, 0.0), couple=1, couple_scale=-1.0 / lz, s=s)
    P = fr.efield("ld", c, (0.0, 0.0, -s / lz))
    assert fr.frac("coupled against the plain field", L.out.v[:10], P.out.v[:10], fr.TOL * P.out.m[:10]) <= 1.0
    D = fr.efield("f64", c, (0.0, 0.0, 0.25), couple=1, couple_scale=-1.0 / lz, s=s)
    assert float(D.E[2]) == fr.QE2F * (0.25 + (-1.0 / lz) * s)
