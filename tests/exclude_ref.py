"""numpy restatement of the two rules of DESIGN.md section 25 (include/conp_hip.h), and the inputs the GPU tests share.

excluded / filter_list: LAMMPS' Neighbor::exclusion(i, j, type_i, type_j, mask, molecule) as conp_pair_build_list_exclude_device
applies it -- a pair is dropped if ex_type[type_i][type_j] is set (every type rule sets both orientations), or some group rule has
mask_i & bit1 and mask_j & bit2 or the same with i and j swapped, or some molecule rule has its bit on both atoms and their
molecule ids equal (intra) or unequal (inter).  mirror_map / mirror_apply: FixZmirror::setup and the one-rank branch of
FixZmirror::post_integrate.  tests/test_exclude_ref_math.py checks this module without a GPU."""
from types import SimpleNamespace

import numpy as np

from conp_amd import neighbor

NEIGHMASK = 0x3FFFFFFF
ALL, PARITY, UPPER, THIRD = 1, 2, 4, 8          # the synthetic groups' bit masks (bits 0 .. 3)


def rules(ntypes=0, type_pairs=(), group_pairs=(), molecule=()):
    """type_pairs [(ti, tj)] 1-based, group_pairs [(bit1, bit2)] bit masks, molecule [(bit, intra)]"""
    return SimpleNamespace(ntypes=ntypes, type_pairs=tuple(type_pairs), group_pairs=tuple(group_pairs), molecule=tuple(molecule))


def excluded(i, j, r, type, mask, molecule):
    """True where the pair (i[k], j[k]) is dropped"""
    i, j = np.asarray(i, dtype=np.int64), np.asarray(j, dtype=np.int64)
    out = np.zeros(i.shape, dtype=bool)
    if r.type_pairs:
        ex = np.zeros((r.ntypes + 1, r.ntypes + 1), dtype=bool)
        for ti, tj in r.type_pairs:
            ex[ti, tj] = ex[tj, ti] = True
        out |= ex[np.clip(type[i], 0, r.ntypes), np.clip(type[j], 0, r.ntypes)]
    for b1, b2 in r.group_pairs:
        out |= ((mask[i] & b1) != 0) & ((mask[j] & b2) != 0)
        out |= ((mask[i] & b2) != 0) & ((mask[j] & b1) != 0)
    for bit, intra in r.molecule:
        both = ((mask[i] & bit) != 0) & ((mask[j] & bit) != 0)
        same = molecule[i] == molecule[j]
        out |= both & (same if intra else ~same)
    return out


def filter_list(lst, r, type, mask, molecule):
    """`lst` (rows following each other in ilist order) without its excluded entries, the order inside every row kept; the special
    bits of the entries that stay are kept"""
    own = np.asarray(lst.ilist[:lst.inum], dtype=np.int64)
    cnt = lst.numneigh[own].astype(np.int64)
    i = np.repeat(own, cnt)
    start = np.repeat(lst.first[own].astype(np.int64), cnt)
    within = np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    entry = lst.neigh[start + within]
    j = entry.astype(np.int64) & NEIGHMASK
    keep = ~excluded(i, j, r, type, mask, molecule)
    numneigh = np.zeros_like(lst.numneigh)
    np.add.at(numneigh, i[keep], 1)
    first = np.zeros_like(lst.first)
    first[own] = (np.cumsum(numneigh[own]) - numneigh[own]).astype(first.dtype)
    return neighbor.NeighList(inum=lst.inum, ilist=lst.ilist.copy(), numneigh=numneigh, first=first,
                              neigh=np.ascontiguousarray(entry[keep]))


def synthetic(at, seed=7):
    """the per-atom class data of the GPU tests: molecule = (tag - 1) // 3 + 1; mask: bit 0 on every atom, bit 1 by the parity of the
    tag, bit 2 on the upper-z half of the owned atoms, bit 3 on a random third; ghost rows copy their owners"""
    n = at.nlocal
    tag = at.tag[:n].astype(np.int64)
    mask = np.full(n, ALL, dtype=np.int32)
    mask[tag % 2 == 1] |= PARITY
    mask[at.x[:n, 2] > np.median(at.x[:n, 2])] |= UPPER
    mask[np.random.default_rng(seed).random(n) < 1.0 / 3.0] |= THIRD
    molecule = ((tag - 1) // 3 + 1).astype(np.int32)
    own = np.asarray(at.owner, dtype=np.int64)
    return SimpleNamespace(type=np.ascontiguousarray(at.type, dtype=np.int32), mask=np.ascontiguousarray(mask[own]),
                           molecule=np.ascontiguousarray(molecule[own]))


def rule_cases(ntypes):
    """the rule kinds of the GPU matrix, by name"""
    each = dict(type_tt=rules(ntypes, type_pairs=[(5, 5)]),
                type_tu=rules(ntypes, type_pairs=[(1, 2)]),
                group_same=rules(group_pairs=[(PARITY, PARITY)]),
                group_overlap=rules(group_pairs=[(UPPER, THIRD)]),
                mol_intra=rules(molecule=[(ALL, 1)]),
                mol_inter=rules(molecule=[(THIRD, 0)]))
    each["all_kinds"] = rules(ntypes, type_pairs=[(5, 5), (1, 2)], group_pairs=[(PARITY, PARITY), (UPPER, THIRD)],
                              molecule=[(ALL, 1), (THIRD, 0)])
    each["sixteen"] = rules(group_pairs=[(PARITY, UPPER), (THIRD, THIRD), (UPPER, THIRD), (PARITY, PARITY)] * 4,
                            molecule=[(ALL, 1), (THIRD, 0), (PARITY, 1), (UPPER, 0)] * 4)
    return each


def mirror_map(tag, mask, groupbit, jgroupbit):
    """(src, dst) owned indices, ascending src: for every atom i of the sending group the atom with tag
    tag[i] - send_mintag + recv_mintag.  ValueError for what conp_zmirror_set_params refuses"""
    tag, mask = np.asarray(tag, dtype=np.int64), np.asarray(mask, dtype=np.int64)
    if len(np.unique(tag)) != len(tag):
        raise ValueError("a tag occurs twice")
    send, recv = (mask & groupbit) != 0, (mask & jgroupbit) != 0
    if not send.any():
        raise ValueError("the sending group is empty")
    if not recv.any():
        raise ValueError("the receiving group is empty")
    smin, smax, rmin, rmax = tag[send].min(), tag[send].max(), tag[recv].min(), tag[recv].max()
    if smax - smin != rmax - rmin:
        raise ValueError("Groups do not have same number of tags")
    at = {int(t): k for k, t in enumerate(tag)}
    src = np.nonzero(send)[0]
    dst = np.empty_like(src)
    for k, i in enumerate(src):
        j = at.get(int(tag[i] - smin + rmin))
        if j is None:
            raise ValueError("no owned atom has the target tag")
        if not recv[j]:
            raise ValueError("a target is outside the receiving group")
        if send[j]:
            raise ValueError("a target is itself in the sending group")
        dst[k] = j
    return src.astype(np.int32), dst.astype(np.int32)


def mirror_groups(n, seed, layout="shuffled"):
    """(tag, mask) of 2 n atoms: the sending group (bit 1) holds tags 1 .. n, the receiving group (bit 2) tags n+1 .. 2n, bit 0 all;
    layout: "shuffled" (tags in random index order), "interleaved" (sender, receiver, sender, ..), "blocks" """
    tag = np.arange(1, 2 * n + 1)
    mask = np.where(tag <= n, 1 | 2, 1 | 4)
    order = {"shuffled": np.random.default_rng(seed).permutation(2 * n), "interleaved": np.arange(2 * n).reshape(2, n).T.ravel(),
             "blocks": np.arange(2 * n)}[layout]
    return tag[order].astype(np.int32), mask[order].astype(np.int32)


def mirror_apply(x, src, dst, zoffset):
    """x with x[dst] = (x[src][0], x[src][1], zoffset - x[src][2]) in float64 as written (the sources are read before any write)"""
    out = np.array(x, dtype=np.float64, copy=True)
    s = out[src].copy()
    out[dst, 0] = s[:, 0]
    out[dst, 1] = s[:, 1]
    out[dst, 2] = np.float64(zoffset) - s[:, 2]
    return out


def cluster(n, nlocal, cutneigh, seed):
    """n atoms inside one sphere of diameter 0.9 cutneigh -- one cell, longer than a wavefront from n = 65 on --, the first nlocal
    owned; tags 1 .. n, the parity group on the odd tags"""
    rng = np.random.default_rng(seed)
    v = rng.normal(size=(n, 3))
    v *= (0.45 * cutneigh * rng.random(n) ** (1.0 / 3.0) / np.linalg.norm(v, axis=1))[:, None]
    tag = np.arange(1, n + 1, dtype=np.int32)
    at = neighbor.Atoms(nlocal=nlocal, nghost=n - nlocal, x=np.ascontiguousarray(v), q=np.zeros(n), type=np.ones(n, np.int32), tag=tag,
                        echeck=np.zeros(n, np.int32), owner=np.arange(n, dtype=np.int32))
    mask = np.where(tag % 2 == 1, ALL | PARITY, ALL).astype(np.int32)
    return at, mask
