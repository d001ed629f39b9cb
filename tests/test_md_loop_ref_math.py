"""Without a GPU: the reference trajectory of tests/md_loop_ref.py has, for every variant and by itself, the properties that
tests/test_gpu_md_loop.py relies on -- so that a device trajectory that differs in the last digits takes the same decisions, and a
passing GPU test has seen re-neighbourings, a changing ghost count, wrapped atoms and molecules across the faces."""
import numpy as np
import pytest

import md_loop_ref as ml


def test_the_starting_system():
    """molecule_system() with its molecules moved apart as rigid bodies: bonds, angles and the face molecules are as they were"""
    import bonded_ref as br
    s0, bonds, angles = br.molecule_system()
    s, b1, a1 = ml.separated_start()
    assert np.array_equal(bonds, b1) and np.array_equal(angles, a1)
    g0, g1 = br._geometry(s0.x, *br._lists(bonds, angles), np.where(s0.periodic, s0.prd, 0.0)), br._geometry(s.x, *br._lists(b1, a1), np.where(s.periodic, s.prd, 0.0))
    assert np.allclose(g0.r, g1.r, atol=1e-12) and np.allclose(g0.c, g1.c, atol=1e-12)
    ele = s.echeck != 0
    assert np.array_equal(s.x[ele], s0.x[ele])
    c = ml.system("A")
    st = ml.straddlers(c, s.x)
    shake = {m for m, _ in ml.SHAKE_MOLS}
    assert set(st) & shake and set(st) - shake and set(st) <= set(ml.FACE_MOLS) | set(st)
    # no two atoms of different molecules closer than R_SEPARATE; the smallest listed distance is a 1-3 distance inside a molecule
    nb = ml.neighbouring(c, s.x)
    i, j = ml.pref.pairs_of(nb.lst)
    sb, j = (j >> 30) & 3, j & ml.pref.NEIGHMASK
    r = np.sqrt(((nb.x[i] - nb.x[j]) ** 2).sum(axis=1))
    mobile = (c.s.echeck[nb.full][i] == 0) | (c.s.echeck[nb.full][j] == 0)              # (the electrode's own bonds are 1.43 A)
    assert r[(sb == 0) & mobile].min() >= ml.R_SEPARATE - 1e-12 and r.min() == ml.min_start() and sb[np.argmin(r)] == 2
    # every flag, the 1 / 3 / 2 mix, and no spring on a constrained bond
    assert sorted(set(c.shake.cluster[:, 0])) == [1, 2, 3]
    constrained = {(int(r_[1]), int(r_[2])) for r_ in c.shake.cluster} | {(int(r_[1]), int(r_[3])) for r_ in c.shake.cluster if r_[0] != 2}
    assert not constrained & {(int(b[0]), int(b[1])) for b in c.bonds}
    assert c.integ.dof[0] == 3 * 64 - 3 - sum({2: 1, 3: 2, 1: 3}[int(f)] for f in c.shake.cluster[:, 0])


@pytest.mark.parametrize("variant", sorted(ml.VARIANTS))
def test_the_reference_trajectory_meets_the_conditions(variant):
    c = ml.system(variant)
    r = ml.reference_trajectory(variant)
    assert len(r.flags) == ml.STEPS <= 40
    assert sum(r.flags) >= 2                                                   # flag-triggered re-neighbourings
    assert len(r.builds) == 1 + sum(r.flags) and [b.step for b in r.builds[1:]] == [k for k, f in enumerate(r.flags) if f]
    counts = [b.nghost for b in r.builds]
    assert any(a != b for a, b in zip(counts, counts[1:]))                     # nghost changes at a re-neighbouring
    assert any(len(b.changed) for b in r.builds[1:])                           # an owned atom's image counter changes at a wrap
    shake = {m for m, _ in ml.SHAKE_MOLS}
    assert any(set(b.straddlers) & shake for b in r.builds[1:]) and any(set(b.straddlers) - shake for b in r.builds[1:])
    margin = np.abs(np.array(r.disp) - c.trigger).min()
    print(f"variant {variant}: re-neighbourings at {[b.step for b in r.builds[1:]]}, nghost {counts}, closest to skin / 2: {margin:.3g} A")
    assert margin >= 1e-6
    assert min(b.cutoff_margin for b in r.builds) >= 1e-9 and min(b.ghost_margin for b in r.builds) >= 1e-9
    assert all(u == 0 and b == 0 and 0 < it <= c.shake.max_iter for u, b, it in r.shake)
    assert r.near > 1e-9                                                       # (the counters of tests/shake_ref.py are equal in both number types)
    assert min(r.rmin) >= ml.min_start()
    assert np.max(r.check) < 0.05 * c.shake.tolerance                          # conp_shake_check_device after every initial integrate
    if c.integ.style[0]:
        assert abs(r.state[0, 3]) > 1e-7                                       # ... under a chain that does act: eta_dot[0], 1 / fs
    if variant in ml.GATE_OPEN:
        assert max(r.gate) >= 4
    else:
        assert not any(r.gate)
    if c.mirror is not None:                                                   # the mirror relation holds at the end, the images stay inside the box
        m = c.mirror
        assert np.array_equal(r.x[m.dst, 2], m.zoffset - r.x[m.src, 2]) and np.array_equal(r.x[m.dst, :2], r.x[m.src, :2])
        assert np.all(c.integ.group[m.dst] == -1) and not c.shake.member[np.concatenate([m.src, m.dst])].any()
        assert np.abs(r.x[m.dst, 2]).max() < c.s.boxhi[2] - 1.0 and np.abs(r.x[m.src] - c.s.x[m.src]).max() > 0.5
        nb = ml.neighbouring(c, c.s.x)
        assert 0 < nb.lst.neigh.size < nb.npairs_plain
    ld = ml.reference_trajectory(variant, kind="ld")
    assert ld.flags == r.flags and ld.nghost == r.nghost and np.array_equal(ld.image, r.image)
