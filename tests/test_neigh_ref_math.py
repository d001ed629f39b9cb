"""no GPU needed: the reference list of tests/neigh_ref.py -- what tests/test_gpu_pair_build_list.py compares the device build with --
against neighbor.build_lists, its special-bond rule on hand-made tables, and the properties the GPU inputs must have (the table in
DESIGN.md section 17)."""
import numpy as np
import pytest

import neigh_ref as nref
import pair_force_ref as pref
from conp_amd import neighbor

NEIGHMASK = 0x3FFFFFFF
CASES = [("small", False), ("small", True), ("small127", False), ("small127", True), ("sparse", False), ("sparse", True),
         ("dilute", False), ("dilute", True), ("il_onelayer", False)]
PAIRS = {("small", False): 30749, ("small", True): 18357, ("sparse", False): 4795, ("sparse", True): 2953,
         ("dilute", False): 17969, ("dilute", True): 12742, ("il_onelayer", False): 2677267}


def _pairset(lst):
    i, j = pref.pairs_of(lst)
    return set(zip(i.tolist(), j.tolist()))


@pytest.mark.parametrize("kind,newton", [c for c in CASES if c[0] != "small127"])
def test_without_a_table_it_is_the_list_of_build_lists(kind, newton):
    inp = nref.inputs(kind, newton)
    at, lst, _ = neighbor.build_lists(inp.s)
    assert at.nall == inp.at.nall and np.array_equal(at.x, inp.at.x)
    ref, _ = nref.reference(inp)
    assert _pairset(ref) == _pairset(lst)
    assert ref.neigh.size == lst.neigh.size == PAIRS[(kind, newton)]
    n = at.nlocal
    assert np.array_equal(ref.ilist, np.arange(n)) and np.all(ref.numneigh[n:] == 0) and np.all(ref.first[n:] == 0)
    assert np.array_equal(ref.first[:n], np.cumsum(ref.numneigh[:n]) - ref.numneigh[:n])
    assert np.array_equal(nref.sort_rows(n, ref.numneigh, ref.neigh), ref.neigh)          # its rows are sorted already


@pytest.mark.parametrize("kind,newton", CASES)
def test_gpu_inputs_keep_their_distance_from_the_cutoff(kind, newton):
    inp = nref.inputs(kind, newton)
    m = nref.cutoff_margin(inp)
    print(f"{kind}: nlocal {inp.at.nlocal} + nghost {inp.at.nghost}, cutneigh {inp.cutneigh}, min |r - cutneigh| = {m:.3g}")
    assert m >= 1e-9


def test_gpu_inputs_have_the_rows_and_boxes_the_kernels_can_go_wrong_on():
    small, sparse = nref.inputs("small", True), nref.inputs("sparse", True)
    at = small.at
    # the small box is narrower than cutneigh: every atom is a neighbour of its own images
    assert np.all(np.asarray(small.s.prd)[:2] < small.cutneigh)
    ref, d = nref.reference(nref.inputs("small", False))
    own_image = at.owner[d.entry & NEIGHMASK] == d.i
    assert set(d.i[own_image].tolist()) == set(range(at.nlocal))
    # rows longer than a wavefront with a ragged last pass, shorter than one, and empty ones
    nn_off = ref.numneigh[:at.nlocal]
    assert np.any((nn_off > 64) & (nn_off % 64 != 0))
    nn_sparse = nref.reference(sparse)[0].numneigh[:sparse.at.nlocal]
    assert np.any(nn_sparse == 0) and np.any((nn_sparse > 0) & (nn_sparse < 64))
    # the sparse box: far more cutneigh-sized cells than occupied ones
    ext = sparse.at.x.max(axis=0) - sparse.at.x.min(axis=0)
    cells = np.maximum(np.floor(ext / sparse.cutneigh), 1).astype(int)
    occupied = len(np.unique(np.minimum(np.floor((sparse.at.x - sparse.at.x.min(axis=0)) / sparse.cutneigh).astype(int), cells - 1), axis=0))
    assert ext[2] > 170 and occupied < np.prod(cells)
    # graphene atoms share one z: the newton-on tie-break of an owned-ghost pair goes to y, and to x
    x = at.x
    _, dn = nref.reference(small)
    j = dn.entry & NEIGHMASK
    g = j >= at.nlocal
    same_z = g & (x[j, 2] == x[dn.i, 2])
    assert np.any(same_z & (x[j, 1] != x[dn.i, 1])) and np.any(same_z & (x[j, 1] == x[dn.i, 1]))
    assert nref.inputs("small127", False).at.nlocal == 127 and nref.inputs("small127", False).at.nlocal % 4 != 0


def _tiny():
    """two owned atoms and one ghost (an image of atom 1) on a line, tags 1, 2, 2"""
    x = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [-9.0, 0.0, 0.0]])
    at = neighbor.Atoms(nlocal=2, nghost=1, x=x, q=np.zeros(3), type=np.ones(3, np.int32), tag=np.array([1, 2, 2], np.int32),
                        echeck=np.zeros(3, np.int32), owner=np.array([0, 1, 1], np.int32))
    return at


def test_the_bits_follow_the_class_of_the_first_match():
    at = _tiny()
    i, j = np.array([0, 0]), np.array([1, 2])
    special = np.array([[9, 2, 2, 2], [1, 0, 0, 0]], np.int32)
    for n, want in (((1, 2, 4), 2), ((2, 3, 4), 1), ((1, 1, 4), 3), ((0, 0, 4), 3), ((1, 1, 1), 0), ((0, 0, 0), 0)):
        nspecial = np.array([n, (1, 1, 1)], np.int32)
        bits, d = nref.special_bits(at, i, j, nspecial, special, pref.SPECIAL_LJ, pref.SPECIAL_COUL, (0.0, 0.0, 0.0))
        assert (bits >> 30).tolist() == [want, want], (n, bits)               # the ghost carries its owner's tag: the same class


def test_the_half_box_rule_strips_the_bits():
    at = _tiny()
    i, j = np.array([0, 0]), np.array([1, 2])
    nspecial, special = np.array([(1, 1, 1), (1, 1, 1)], np.int32), np.array([[2], [1]], np.int32)
    bits, d = nref.special_bits(at, i, j, nspecial, special, pref.SPECIAL_LJ, pref.SPECIAL_COUL, (5.0, 5.0, 5.0))
    assert (bits >> 30).tolist() == [1, 0] and d.image.tolist() == [False, True]      # |del_x| = 9 > 5: an ordinary neighbour
    bits, _ = nref.special_bits(at, i, j, nspecial, special, pref.SPECIAL_LJ, pref.SPECIAL_COUL, (0.0, 5.0, 5.0))
    assert (bits >> 30).tolist() == [1, 1]                                            # x not periodic: no check along it
    bits, _ = nref.special_bits(at, i, j, nspecial, special, pref.SPECIAL_LJ, pref.SPECIAL_COUL, (9.0, 5.0, 5.0))
    assert (bits >> 30).tolist() == [1, 1]                                            # exactly half a box: kept (LAMMPS tests `>`)


def test_factors_that_are_both_one_strip_the_bits():
    at = _tiny()
    i, j = np.array([0, 0]), np.array([1, 2])
    special = np.array([[2], [1]], np.int32)
    for cls in (1, 2, 3):
        nspecial = np.array([[(1, 1, 1), (0, 1, 1), (0, 0, 1)][cls - 1], (0, 0, 0)], np.int32)
        lj, coul = [1.0, 0.0, 0.0, 0.5], [1.0, 0.0, 0.5, 0.8333]
        bits, _ = nref.special_bits(at, i, j, nspecial, special, lj, coul, (0.0, 0.0, 0.0))
        assert (bits >> 30).tolist() == [cls, cls]
        lj[cls] = 1.0
        bits, _ = nref.special_bits(at, i, j, nspecial, special, lj, coul, (0.0, 0.0, 0.0))
        assert (bits >> 30).tolist() == [cls, cls]                                    # only one of the two is 1.0
        coul[cls] = 1.0
        bits, _ = nref.special_bits(at, i, j, nspecial, special, lj, coul, (0.0, 0.0, 0.0))
        assert (bits >> 30).tolist() == [0, 0]


@pytest.mark.parametrize("newton", [False, True])
def test_the_chain_table_shows_every_case(newton):
    inp = nref.inputs("small", newton)
    at = inp.at
    sp = nref.chain_specials(at)
    assert sp[0].max() < nref.MAXSPECIAL and np.all(np.diff(sp[0], axis=1) >= 0)
    ref, d = nref.reference(inp, sp, pref.SPECIAL_LJ, pref.SPECIAL_COUL)
    plain, _ = nref.reference(inp)
    assert np.array_equal(ref.numneigh, plain.numneigh)                               # nothing is dropped
    which = (d.entry >> 30) & 3
    j = d.entry & NEIGHMASK
    assert {1, 2, 3} <= set(which.tolist())
    assert np.any((which > 0) & (j >= at.nlocal))                                     # a ghost entry with bits
    det = d.detail
    stripped = (det.which[d.order] > 0) & det.image[d.order]
    assert np.any(stripped) and np.all(which[stripped] == 0)                          # an image of a partner, more than half a box away
    # the repeated 1-2 tag at the end of the 1-4 block never decides: no pair is class 3 whose tag is a 1-2 partner
    n1 = sp[0][d.i, 0]
    in12 = (sp[1][d.i] == at.tag[j][:, None]) & (np.arange(nref.MAXSPECIAL)[None, :] < n1[:, None])
    assert np.any(in12.any(axis=1)) and np.all(det.which[d.order][in12.any(axis=1)] == 1)
    # all factors 1.0: no bits at all
    none, _ = nref.reference(inp, sp, pref.ONES, pref.ONES)
    assert np.array_equal(none.neigh, plain.neigh)
