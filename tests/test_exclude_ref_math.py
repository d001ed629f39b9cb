"""no GPU: tests/exclude_ref.py -- the exclusion rule and the mirror map the GPU tests of DESIGN.md section 25 compare with.

(1) filter_list of neigh_ref.reference against an O(n^2) brute force of the rule written with plain loops over the rules, for each
rule kind;  (2) a group rule with bit1 != bit2 is symmetric in i and j;  (3) intra plus inter on one bit removes every pair inside
that group;  (4) every rule of the GPU matrix removes at least one pair and leaves at least one, on every input of that matrix;
(5) mirror_apply twice with swapped groups returns the input bits when zoffset = 0;  (6) each refusal of mirror_map."""
import numpy as np
import pytest

import exclude_ref as xref
import neigh_ref as nref

KINDS = ("small", "small127", "sparse")


def _brute(inp, r, cls):
    """the listed pairs (i, j), i < nlocal, straight from the set rule of conp_pair_build_list_device and the exclusion rule, pair by pair"""
    at = inp.at
    x, n = at.x, at.nlocal
    ex_type = set()
    for ti, tj in r.type_pairs:
        ex_type |= {(ti, tj), (tj, ti)}
    out = []
    for i in range(n):
        d = x[i] - x
        rsq = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
        for j in np.nonzero(rsq < inp.cutneigh * inp.cutneigh)[0]:
            if j == i:
                continue
            if j < n or not inp.newton:
                ok = j > i
            else:
                ok = (x[j, 2], x[j, 1], x[j, 0]) > (x[i, 2], x[i, 1], x[i, 0])
            if not ok:
                continue
            mi, mj = int(cls.mask[i]), int(cls.mask[j])
            drop = (int(cls.type[i]), int(cls.type[j])) in ex_type
            for b1, b2 in r.group_pairs:
                drop = drop or bool(mi & b1 and mj & b2) or bool(mi & b2 and mj & b1)
            for bit, intra in r.molecule:
                if mi & bit and mj & bit:
                    same = cls.molecule[i] == cls.molecule[j]
                    drop = drop or bool(same if intra else not same)
            if not drop:
                out.append((i, int(j)))
    return sorted(out)


def _pairs(lst):
    i = np.repeat(np.arange(lst.inum), lst.numneigh[:lst.inum])
    return sorted(zip(i.tolist(), (lst.neigh.astype(np.int64) & xref.NEIGHMASK).tolist()))


@pytest.mark.parametrize("newton", [False, True])
@pytest.mark.parametrize("name", ["type_tt", "type_tu", "group_same", "group_overlap", "mol_intra", "mol_inter", "all_kinds", "sixteen"])
def test_filter_list_is_the_brute_force_of_the_rule(name, newton):
    inp = nref.inputs("small", newton)
    cls = xref.synthetic(inp.at)
    r = xref.rule_cases(inp.s.ntypes)[name]
    ref = nref.reference(inp)[0]
    got = xref.filter_list(ref, r, cls.type, cls.mask, cls.molecule)
    assert _pairs(got) == _brute(inp, r, cls)
    n = inp.at.nlocal
    assert np.array_equal(got.first[:n], np.cumsum(got.numneigh[:n]) - got.numneigh[:n]) and got.numneigh[:n].sum() == got.neigh.size
    assert np.all(got.numneigh[n:] == 0)
    # the order inside a row is kept: the filtered row is a subsequence of the reference's row
    for i in (0, 5, n - 1):
        a = ref.neigh[ref.first[i]:ref.first[i] + ref.numneigh[i]].tolist()
        b = got.neigh[got.first[i]:got.first[i] + got.numneigh[i]].tolist()
        it = iter(a)
        assert all(v in it for v in b)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("newton", [False, True])
def test_every_rule_of_the_gpu_matrix_removes_a_pair_and_leaves_one(kind, newton):
    inp = nref.inputs(kind, newton)
    assert nref.cutoff_margin(inp) >= 1e-9
    cls = xref.synthetic(inp.at)
    for special in (False, True):
        sp = nref.chain_specials(inp.at) if special else None
        ref = nref.reference(inp, sp, *((nref.pref.SPECIAL_LJ, nref.pref.SPECIAL_COUL) if special else (nref.pref.ONES, nref.pref.ONES)))[0]
        for name, r in xref.rule_cases(inp.s.ntypes).items():
            got = xref.filter_list(ref, r, cls.type, cls.mask, cls.molecule)
            assert 0 < got.neigh.size < ref.neigh.size, (kind, newton, name, got.neigh.size, ref.neigh.size)
            if special:
                assert np.any(got.neigh.astype(np.int64) & ~xref.NEIGHMASK & 0xFFFFFFFF), (kind, name)      # bits survive on kept entries


def test_a_group_rule_is_symmetric_in_i_and_j():
    rng = np.random.default_rng(3)
    n = 200
    mask = rng.integers(0, 16, n).astype(np.int32)
    typ, mol = np.ones(n, np.int32), np.ones(n, np.int32)
    i, j = rng.integers(0, n, 5000), rng.integers(0, n, 5000)
    r = xref.rules(group_pairs=[(xref.UPPER, xref.THIRD)])
    a = xref.excluded(i, j, r, typ, mask, mol)
    assert np.array_equal(a, xref.excluded(j, i, r, typ, mask, mol))
    assert np.array_equal(a, xref.excluded(i, j, xref.rules(group_pairs=[(xref.THIRD, xref.UPPER)]), typ, mask, mol))
    one_way = ((mask[i] & xref.UPPER) != 0) & ((mask[j] & xref.THIRD) != 0)
    assert a.any() and not a.all() and np.any(a & ~one_way)          # the swapped orientation alone drops pairs too


def test_intra_plus_inter_on_one_bit_removes_every_pair_inside_the_group():
    inp = nref.inputs("small", False)
    cls = xref.synthetic(inp.at)
    ref = nref.reference(inp)[0]
    got = xref.filter_list(ref, xref.rules(molecule=[(xref.THIRD, 1), (xref.THIRD, 0)]), cls.type, cls.mask, cls.molecule)
    same = xref.filter_list(ref, xref.rules(group_pairs=[(xref.THIRD, xref.THIRD)]), cls.type, cls.mask, cls.molecule)
    assert got.neigh.tobytes() == same.neigh.tobytes() and np.array_equal(got.numneigh, same.numneigh)
    i = np.repeat(np.arange(got.inum), got.numneigh[:got.inum])
    assert not np.any((cls.mask[i] & xref.THIRD != 0) & (cls.mask[got.neigh] & xref.THIRD != 0))
    assert 0 < got.neigh.size < ref.neigh.size


def test_a_type_outside_the_table_is_clamped():
    r = xref.rules(5, type_pairs=[(5, 5)])
    typ = np.array([5, 9, -3, 0], dtype=np.int32)
    z = np.zeros(4, np.int32)
    assert xref.excluded([0, 0, 0, 0], [0, 1, 2, 3], r, typ, z, z).tolist() == [True, True, False, False]


_two_groups = xref.mirror_groups


def test_mirroring_twice_with_swapped_groups_returns_the_input():
    tag, mask = _two_groups(65, 1)
    x = np.random.default_rng(2).normal(size=(len(tag) + 3, 3)) * 7.0
    s1, d1 = xref.mirror_map(tag, mask, 2, 4)
    s2, d2 = xref.mirror_map(tag, mask, 4, 2)
    assert np.array_equal(tag[d1] - tag[s1], np.full(65, 65)) and np.array_equal(np.sort(s1), s1)
    assert np.array_equal(np.sort(d2), np.sort(s1))
    y = xref.mirror_apply(x, s1, d1, 0.0)
    assert y[s1].tobytes() == x[s1].tobytes() and y[len(tag):].tobytes() == x[len(tag):].tobytes()
    assert np.array_equal(y[d1, 2], -x[s1, 2]) and np.array_equal(y[d1, :2], x[s1, :2])
    back = xref.mirror_apply(y, s2, d2, 0.0)
    assert back[s1].tobytes() == x[s1].tobytes()                    # -(-z) == z bit for bit
    z = xref.mirror_apply(x, s1, d1, 2 * -3.5 + 11.0)
    assert np.array_equal(z[d1, 2], 4.0 - x[s1, 2])


def test_mirror_map_refusals():
    tag, mask = _two_groups(8, 4)
    ok = xref.mirror_map(tag, mask, 2, 4)
    assert len(ok[0]) == 8
    bad = {}
    t = tag.copy(); t[0] = t[1]
    bad["twice"] = (t, mask, 2, 4)
    bad["sending group is empty"] = (tag, mask, 16, 4)
    bad["receiving group is empty"] = (tag, mask, 2, 16)
    m = mask.copy(); m[tag == 16] = 1                                # the receiving range shrinks to 9 .. 15
    bad["same number of tags"] = (tag, m, 2, 4)
    t = tag.copy(); t[tag == 12] = 16; t[tag == 16] = 12                       # (two receivers swap tags: still fine)
    assert len(xref.mirror_map(t, mask, 2, 4)[0]) == 8
    t = tag.copy(); t[tag == 12] = 100; m = mask.copy(); m[tag == 12] = 1      # tag 12 is gone, the ranges still agree
    bad["no owned atom"] = (t, m, 2, 4)
    m = mask.copy(); m[tag == 12] = 1                               # tag 12 exists but left the receiving group
    bad["outside the receiving group"] = (tag, m, 2, 4)
    # sending = tags 1 .. 8, receiving = tags 5 .. 12: equal ranges, and the target of tag 1 (tag 5) is itself a sender
    tag3 = np.arange(1, 13).astype(np.int32)
    mask3 = np.where(tag3 <= 4, 1 | 2, np.where(tag3 <= 8, 1 | 2 | 4, 1 | 4)).astype(np.int32)
    bad["itself in the sending group"] = (tag3, mask3, 2, 4)
    for text, args in bad.items():
        with pytest.raises(ValueError, match=text):
            xref.mirror_map(*args)
    assert np.array_equal(xref.mirror_map(tag, mask, 2, 4)[1], ok[1])
