"""no GPU needed: the numpy reference of the ghost entries (tests/ghost_ref.py, written from include/conp_hip.h) against
conp_amd/neighbor.py::make_ghosts, and its fold and remap on hand-made cases.  tests/test_gpu_ghosts.py compares the device with it."""
import numpy as np
import pytest

import ghost_ref as gref
import neigh_ref as nref
from conp_amd import neighbor

KINDS = ["small", "sparse", "dilute", "il_onelayer"]


@pytest.mark.parametrize("kind", KINDS)
def test_build_is_make_ghosts(kind):
    inp = nref.inputs(kind, False)
    s, at = inp.s, neighbor.make_ghosts(inp.s)
    boxlo, boxhi, periodic, cut = gref.box_of(s)
    assert cut == inp.cutneigh
    r = gref.build(s.x, boxlo, boxhi, periodic, cut)
    n = at.nlocal
    assert (r.nlocal, r.nghost) == (n, at.nghost)
    assert np.array_equal(r.owner, at.owner[n:])                     # the same ghosts in the same order
    assert np.array_equal(r.x, at.x)                                 # ... with the same bits
    assert np.array_equal(r.x[n:], at.x[r.owner] + r.img * r.prd)
    print(f"{kind}: {n} owned, {r.nghost} ghosts, {r.nshift} shifts, margin {r.margin:.3g} A")
    assert r.margin >= 1e-9                                          # `<` against `<=`, or a rounding, cannot change the set
    per_owner = np.bincount(r.owner, minlength=n)
    if kind == "small":
        prd = r.prd
        assert cut > prd[0] and cut > prd[1] and cut < prd[2]        # m = (2, 2, 1)
        assert r.nshift == 5 * 5 * 3 - 1 == 74
        assert per_owner.min() >= 8 and per_owner.max() <= 15 and per_owner.max() > per_owner.min()
        assert np.abs(r.img[:, :2]).max() == 2
    if kind == "sparse":
        assert tuple(periodic) == (True, True, False) and np.all(r.img[:, 2] == 0)
    # an owner's ghosts ascend with the shift index: no sort is needed for its list
    order = np.argsort(r.owner, kind="stable")
    assert np.all(np.diff(order)[np.diff(r.owner[order]) == 0] > 0)


def test_small127_is_the_build_of_the_first_127_atoms():
    inp = nref.inputs("small127", False)
    boxlo, boxhi, periodic, cut = gref.box_of(inp.s)
    r = gref.build(inp.s.x[:127], boxlo, boxhi, periodic, cut)
    assert inp.at.nlocal == 127 and np.array_equal(r.x, inp.at.x) and np.array_equal(r.owner, inp.at.owner[127:])


def test_a_coordinate_that_is_not_finite_has_no_images():
    inp = nref.inputs("small", False)
    boxlo, boxhi, periodic, cut = gref.box_of(inp.s)
    base = gref.build(inp.s.x, boxlo, boxhi, periodic, cut)
    x = inp.s.x.copy()
    x[5, 0], x[5, 1] = np.nan, np.inf
    r = gref.build(x, boxlo, boxhi, periodic, cut)
    assert np.any(base.owner == 5) and not np.any(r.owner == 5)
    assert np.array_equal(r.owner, base.owner[base.owner != 5]) and np.array_equal(r.img, base.img[base.owner != 5])


def test_fold_on_three_atoms():
    """two owned atoms, four ghosts: owner 0 has ghosts 0, 2, 3 (in that order), owner 1 has ghost 1.  The values are chosen so that
    the order of the sum shows: (1 + 1e16) - 1e16 = 0 in double, 1 + (1e16 - 1e16) = 1"""
    owner = np.array([0, 1, 0, 0])
    v = np.array([1.0, 5.0, 1e16, 0.25, -1e16, 3.0])
    out = gref.fold(v, owner, 2)
    assert out[0] == ((1.0 + 1e16) + -1e16) + 3.0 == 3.0
    assert out[1] == 5.25
    assert np.array_equal(out[2:], v[2:])                            # ghost rows stay
    v3 = np.stack([v, 2 * v, -v], axis=1)
    out3 = gref.fold(v3, owner, 2)
    assert np.array_equal(out3[:, 0], out) and np.array_equal(out3[:, 1], 2 * out) and np.array_equal(out3[:, 2], -out)
    assert np.array_equal(gref.fold(v[:2], np.zeros(0, np.int64), 2), v[:2])         # no ghosts: nothing to add


def test_wrap_edges():
    e = gref.edge_case()
    prd1 = e.boxhi[1] - e.boxlo[1]
    assert e.boxhi[1] - prd1 < e.boxlo[1]                            # the subtraction alone would leave the atom outside the box
    assert e.boxhi[0] - (e.boxhi[0] - e.boxlo[0]) == e.boxlo[0]
    x, image = gref.wrap(e.x, e.boxlo, e.boxhi, e.periodic)
    assert np.array_equal(x, e.want_x) and np.array_equal(image, e.want_image)
    assert np.all((x[:, :2] >= e.boxlo[:2]) & (x[:, :2] < e.boxhi[:2]))
    x2, image2 = gref.wrap(x, e.boxlo, e.boxhi, e.periodic, image)   # inside the box: nothing more happens
    assert np.array_equal(x2, x) and np.array_equal(image2, image)
    # below the box, and counters that are added to
    lo, hi = np.array([0.0, 0.0, 0.0]), np.array([10.0, 10.0, 10.0])
    x, image = gref.wrap([[-0.5, 10.5, -3.0]], lo, hi, (True, True, False), np.array([[4, 4, 4]]))
    assert np.array_equal(x, [[9.5, 0.5, -3.0]]) and np.array_equal(image, [[3, 5, 4]])
