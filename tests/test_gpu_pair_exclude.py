"""-m gpu: conp_pair_set_exclusions / conp_pair_build_list_exclude_device -- LAMMPS' neigh_modify exclude in the device list build
 against tests/exclude_ref.py::filter_list of the reference list of tests/neigh_ref.py (both checked without
a GPU by tests/test_exclude_ref_math.py).

(1) every rule kind x newton x special: per-row set equality with the filtered reference, and the arrays byte-equal to the handle's
own plain build with the excluded entries removed in order;  (2) zero rules and a rule that matches no pair: the plain build's bytes;
(3) a rule that matches every pair: an empty, valid list, all pair outputs zero;  (4) compaction edges: one cell of 63 .. 257 atoms,
alternating lanes dropped, rows entry for entry;  (5) two builds, the same bytes; NULL rules then the plain entry; a second set of
rules replaces the first;  (6) pair forces on an excluded list to the bound of tests/test_gpu_pair_forces.py;  (7) the displacement
flag after an excluded build;  (8) every refusal, each followed by a valid call;  (9) on the zmirror deck's box
conp_fix_post_neighbor_device behind an excluded build with the deck's rule: the host route's tables and charges."""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import exclude_ref as xref
import neigh_ref as nref
import pair_force_ref as pref
from conp_amd import ConpError, FixConp, capi, neighbor, systems
from test_gpu_pair_build_list import _dev, _factors, _handle, _reference, _same_list
from test_gpu_pair_device import _call, _to_device
from test_gpu_pair_forces import check, system

pytestmark = pytest.mark.gpu

RULES = ["type_tt", "type_tu", "group_same", "group_overlap", "mol_intra", "mol_inter", "all_kinds", "sixteen"]
INPUTS = [("small", False), ("small", True), ("small127", False), ("small127", True), ("sparse", False), ("sparse", True)]
FIELDS = ("ilist", "numneigh", "first", "neigh")


def _set(fx, r):
    fx.pair_set_exclusions(r.ntypes, r.type_pairs, r.group_pairs, r.molecule)


def _class_arrays(cls):
    return (_dev(cls.type, np.int32), _dev(cls.mask, np.int32), _dev(cls.molecule, np.int32))


def _specials(at, special):
    if not special:
        return {}, None
    nsp, sp = nref.chain_specials(at)
    keep = (_dev(at.tag, np.int32), _dev(nsp, np.int32), _dev(sp, np.int32))
    return dict(d_tag=keep[0].data_ptr(), d_nspecial=keep[1].data_ptr(), d_special=keep[2].data_ptr(), maxspecial=nref.MAXSPECIAL), keep


def _build(fx, inp, d_x, d_cls, special=False, plain=False, **over):
    """one build by the exclude entry (plain: by conp_pair_build_list_device) -> (NeighList, nall)"""
    at = inp.at
    kw, keep = _specials(at, special)
    a = dict(d_x=d_x.data_ptr(), nlocal=at.nlocal, nall=at.nall, cutneigh=inp.cutneigh, prd_half=inp.prd_half, **kw)
    if not plain:
        a.update(d_type=d_cls[0].data_ptr(), d_mask=d_cls[1].data_ptr(), d_molecule=d_cls[2].data_ptr())
    a.update(over)
    (fx.pair_build_list_device if plain else fx.pair_build_list_exclude_device)(**a)
    return fx.pair_get_list()


def _same_bytes(tag, a, b):
    for name in FIELDS:
        assert getattr(a, name).tobytes() == getattr(b, name).tobytes(), (tag, name)


@pytest.mark.parametrize("special", [False, True])
@pytest.mark.parametrize("kind,newton", INPUTS)
def test_every_rule_kind_gives_the_filtered_reference(kind, newton, special):
    inp = nref.inputs(kind, newton)
    assert nref.cutoff_margin(inp) >= 1e-9
    at = inp.at
    cls = xref.synthetic(at)
    fx, _ = _handle(inp.s, special)
    d_x, d_cls = _dev(at.x, np.float64), _class_arrays(cls)
    ref = _reference(inp, special)
    plain, _ = _build(fx, inp, d_x, d_cls, special, plain=True)
    for name in RULES:
        r = xref.rule_cases(inp.s.ntypes)[name]
        want = xref.filter_list(ref, r, cls.type, cls.mask, cls.molecule)
        _set(fx, r)
        got, nall = _build(fx, inp, d_x, d_cls, special)
        print(f"{kind}, newton {newton}, special {special}, {name}: {got.neigh.size} of {ref.neigh.size} pairs")
        assert 0 < want.neigh.size < ref.neigh.size, name                      # the rule removed a pair and left one
        _same_list(f"{kind} {newton} {special} {name}", got, nall, want, at)          # (rows of a filtered sorted list stay sorted)
        _same_bytes(name, got, xref.filter_list(plain, r, cls.type, cls.mask, cls.molecule))
        if special:
            assert np.any(got.neigh.astype(np.int64) & 0xC0000000)
    fx.close()


def test_zero_rules_and_a_rule_without_a_match_give_the_plain_bytes():
    inp = nref.inputs("small", True)
    at, cls = inp.at, xref.synthetic(inp.at)
    fx, _ = _handle(inp.s, True)
    d_x, d_cls = _dev(at.x, np.float64), _class_arrays(cls)
    plain, _ = _build(fx, inp, d_x, d_cls, True, plain=True)
    fx.pair_set_exclusions()                                                   # all counts 0: no per-atom array is needed
    got, _ = _build(fx, inp, d_x, d_cls, True, d_type=0, d_mask=0, d_molecule=0)
    _same_bytes("zero rules", got, plain)
    fx.pair_set_exclusions(clear=True)                                         # NULL: the same
    got, _ = _build(fx, inp, d_x, d_cls, True, d_type=0, d_mask=0, d_molecule=0)
    _same_bytes("NULL rules", got, plain)
    nobody = xref.rules(inp.s.ntypes, group_pairs=[(16, 16), (xref.ALL, 32)], molecule=[(64, 1), (64, 0)])
    assert not xref.excluded(*np.meshgrid(np.arange(50), np.arange(50)), nobody, cls.type, cls.mask, cls.molecule).any()
    _set(fx, nobody)
    got, _ = _build(fx, inp, d_x, d_cls, True)
    _same_bytes("a rule that matches no pair", got, plain)
    fx.close()


def test_a_rule_that_matches_every_pair_leaves_an_empty_valid_list():
    import torch
    inp = nref.inputs("small", False)
    at, cls = inp.at, xref.synthetic(inp.at)
    ref = _reference(inp, False)
    fx, _ = _handle(inp.s, False)
    fx.init_lists(ref, ref)
    fx.setup_post_neighbor(at)
    d_x, d_q = _to_device(at)
    d_cls = _class_arrays(cls)
    _set(fx, xref.rules(group_pairs=[(xref.ALL, xref.ALL)]))
    got, nall = _build(fx, inp, d_x, d_cls)
    assert nall == at.nall and got.inum == at.nlocal and got.neigh.size == 0
    assert np.all(got.numneigh == 0) and np.all(got.first == 0) and np.array_equal(got.ilist, np.arange(at.nlocal))
    f, eng, W, ea, va = _call(fx, d_x, d_q, at.nall)
    assert not np.any(f) and not np.any(eng) and not np.any(W) and not np.any(ea) and not np.any(va)
    fx.close()


@pytest.mark.parametrize("newton", [False, True])
@pytest.mark.parametrize("n", [63, 64, 65, 129, 257])
def test_compaction_edges_in_one_long_cell(n, newton):
    """one cutoff sphere of n atoms: a single cell, longer than a wavefront from 65 on; the parity rule drops alternating lanes.  The
    expected row is written down entry by entry: the cell's members in ascending index"""
    s = system("small", newton)
    cutneigh = float(s.cutoff + s.skin)
    r = xref.rules(group_pairs=[(xref.PARITY, xref.PARITY)])
    fx, _ = _handle(s, False)
    _set(fx, r)
    for nlocal in (1, 3, 4, 5, n):
        at, mask = xref.cluster(n, nlocal, cutneigh, seed=n)
        inp = SimpleNamespace(s=s, at=at, cutneigh=cutneigh, newton=newton, prd_half=np.zeros(3))
        assert nref.cutoff_margin(inp) >= 1e-9
        d_x, d_mask = _dev(at.x, np.float64), _dev(mask, np.int32)
        fx.pair_build_list_exclude_device(d_x.data_ptr(), nlocal, n, cutneigh, d_mask=d_mask.data_ptr())
        got, nall = fx.pair_get_list()
        x = at.x
        rows, dropped = [], 0
        for i in range(nlocal):
            row = []
            for j in range(n):
                if j == i:
                    continue
                if j < nlocal or not newton:
                    ok = j > i
                else:
                    ok = (x[j, 2], x[j, 1], x[j, 0]) > (x[i, 2], x[i, 1], x[i, 0])
                if ok and mask[i] & mask[j] & xref.PARITY:
                    dropped += 1
                elif ok:
                    row.append(j)
            rows.append(row)
        want = np.array([j for row in rows for j in row], dtype=np.int32)
        assert dropped > 0 or nlocal == 1
        assert want.size > 0
        assert nall == n and got.inum == nlocal
        assert np.array_equal(got.numneigh[:nlocal], [len(row) for row in rows]) and np.all(got.numneigh[nlocal:] == 0), (n, nlocal)
        assert np.array_equal(got.neigh, want), (n, nlocal)                     # entry for entry
        assert np.array_equal(got.first[:nlocal], np.cumsum(got.numneigh[:nlocal]) - got.numneigh[:nlocal])
    fx.close()


def test_two_builds_null_rules_and_replaced_rules():
    inp = nref.inputs("small127", True)
    at, cls = inp.at, xref.synthetic(inp.at)
    cases = xref.rule_cases(inp.s.ntypes)
    fx, _ = _handle(inp.s, True)
    d_x, d_cls = _dev(at.x, np.float64), _class_arrays(cls)
    ref = _reference(inp, True)
    _set(fx, cases["sixteen"])
    a, _ = _build(fx, inp, d_x, d_cls, True)
    b, _ = _build(fx, inp, d_x, d_cls, True)
    _same_bytes("two builds", a, b)
    _set(fx, cases["type_tu"])                                                 # the second set replaces the first
    c, nall = _build(fx, inp, d_x, d_cls, True)
    _same_list("replaced", c, nall, xref.filter_list(ref, cases["type_tu"], cls.type, cls.mask, cls.molecule), at)
    assert c.neigh.size != a.neigh.size
    fx.pair_set_exclusions(clear=True)                                         # NULL, then the plain entry still works
    p, nall = _build(fx, inp, d_x, d_cls, True, plain=True)
    _same_list("plain after NULL", p, nall, ref, at)
    _set(fx, cases["sixteen"])                                                 # the plain entry ignores rules in force
    p2, _ = _build(fx, inp, d_x, d_cls, True, plain=True)
    _same_bytes("plain entry with rules on the handle", p, p2)
    fx.close()


@pytest.mark.parametrize("newton,special", [(False, False), (True, True)])
def test_pair_forces_and_the_moved_flag_on_an_excluded_list(newton, special):
    import torch
    inp = nref.inputs("small", newton)
    at, cls = inp.at, xref.synthetic(inp.at)
    r = xref.rule_cases(inp.s.ntypes)["all_kinds"]
    ref = _reference(inp, special)
    want = xref.filter_list(ref, r, cls.type, cls.mask, cls.molecule)
    fx, p = _handle(inp.s, special)
    fx.init_lists(ref, ref)
    fx.setup_post_neighbor(at)
    d_x, d_q = _to_device(at)
    d_cls = _class_arrays(cls)
    _set(fx, r)
    got, nall = _build(fx, inp, d_x, d_cls, special)
    _same_list("forces case", got, nall, want, at)
    R = pref.for_atoms(at, want, p, inp.s, newton, *_factors(special))         # the longdouble reference over the filtered pairs
    Rfull = pref.for_atoms(at, ref, p, inp.s, newton, *_factors(special))
    assert R.npairs < Rfull.npairs and abs(R.eng[1] - Rfull.eng[1]) > 1e-6 * Rfull.E_abs
    check(f"excluded list, newton {newton}, special {special}", _call(fx, d_x, d_q, at.nall), R)
    # conp_pair_list_moved_device after an excluded build
    flag = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    skin = inp.s.skin
    for scale, expect in ((0.49, 0), (0.51, 1)):
        x = at.x.copy(); x[3] += scale * skin * np.array([2.0, -1.0, 2.0]) / 3.0
        d = _dev(x, np.float64)
        fx.pair_list_moved_device(d.data_ptr(), 0.5 * skin, flag.data_ptr())
        torch.cuda.synchronize()
        assert int(flag.cpu()[0]) == expect
    fx.close()


def test_refusals_each_followed_by_a_valid_call():
    inp = nref.inputs("small", False)
    at, s, cls = inp.at, inp.s, xref.synthetic(inp.at)
    d_x, d_cls = _dev(at.x, np.float64), _class_arrays(cls)
    cases = xref.rule_cases(s.ntypes)
    good = cases["all_kinds"]
    ref = _reference(inp, False)
    want = xref.filter_list(ref, good, cls.type, cls.mask, cls.molecule)
    fx = FixConp(s)
    for call in (lambda: fx.pair_set_exclusions(), lambda: _build(fx, inp, d_x, d_cls)):          # before conp_pair_set_params
        with pytest.raises(ConpError) as e:
            call()
        assert e.value.code == -2
    fx.close()
    fx, _ = _handle(s, False)
    with pytest.raises(ConpError) as e:                                          # the build entry before conp_pair_set_exclusions
        _build(fx, inp, d_x, d_cls)
    assert e.value.code == -2 and "before conp_pair_set_exclusions" in str(e.value)

    def valid():
        _set(fx, good)
        got, nall = _build(fx, inp, d_x, d_cls)
        _same_list("after a refusal", got, nall, want, at)
    valid()
    nt = s.ntypes
    seventeen = [(xref.PARITY, xref.PARITY)] * 17
    bad_rules = [dict(ntypes=nt, type_pairs=[(0, 1)]), dict(ntypes=nt, type_pairs=[(1, nt + 1)]), dict(ntypes=nt, type_pairs=[(-1, 1)]),
                 dict(ntypes=nt + 1, type_pairs=[(1, 1)]), dict(ntypes=nt - 1, type_pairs=[(1, 1)]),
                 dict(group_pairs=seventeen), dict(molecule=[(xref.ALL, 1)] * 17),
                 dict(group_pairs=[(0, xref.ALL)]), dict(group_pairs=[(xref.ALL, 0)]), dict(molecule=[(0, 1)])]
    for kw in bad_rules:
        with pytest.raises(ConpError) as e:
            fx.pair_set_exclusions(**kw)
        assert e.value.code == -1, kw
        with pytest.raises(ConpError) as e:                                      # a refused call leaves the handle without rules
            _build(fx, inp, d_x, d_cls)
        assert e.value.code == -2, kw
        valid()
    # negative counts and a count > 0 with a NULL array: the struct by hand
    one = (capi.C.c_int * 1)(1)
    ip = lambda a: capi.C.cast(a, capi.C.POINTER(capi.C.c_int))
    structs = [capi.conp_pair_exclusions(ntypes=nt, ntype_pairs=-1), capi.conp_pair_exclusions(ngroup_pairs=-1),
               capi.conp_pair_exclusions(nmol=-1), capi.conp_pair_exclusions(ntypes=nt, ntype_pairs=1, type_i=ip(one)),
               capi.conp_pair_exclusions(ntypes=nt, ntype_pairs=1, type_j=ip(one)),
               capi.conp_pair_exclusions(ngroup_pairs=1, group_bit1=ip(one)), capi.conp_pair_exclusions(ngroup_pairs=1, group_bit2=ip(one)),
               capi.conp_pair_exclusions(nmol=1, mol_bit=ip(one)), capi.conp_pair_exclusions(nmol=1, mol_intra=ip(one))]
    for st in structs:
        assert fx.lib.conp_pair_set_exclusions(fx.h, capi.C.byref(st)) == -1
        with pytest.raises(ConpError) as e:
            _build(fx, inp, d_x, d_cls)
        assert e.value.code == -2
        valid()
    # the build entry: a NULL at, a NULL array a rule in force needs, and the plain entry's refusals
    a = capi.conp_pair_build_args(nlocal=at.nlocal, nall=at.nall, cutneigh=inp.cutneigh)
    assert fx.lib.conp_pair_build_list_exclude_device(fx.h, capi.C.c_void_p(d_x.data_ptr()), capi.C.byref(a), None) == -1
    valid()
    needs = [("type_tt", dict(d_type=0)), ("group_same", dict(d_mask=0)), ("mol_intra", dict(d_mask=0)), ("mol_intra", dict(d_molecule=0)),
             ("all_kinds", dict(d_type=0)), ("all_kinds", dict(d_molecule=0))]
    for name, kw in needs:
        _set(fx, cases[name])
        with pytest.raises(ConpError) as e:
            _build(fx, inp, d_x, d_cls, **kw)
        assert e.value.code == -1, (name, kw)
        with pytest.raises(ConpError) as e:                                      # a refused build leaves the handle without a list
            fx.pair_get_list()
        assert e.value.code == -2
        valid()
    _set(fx, cases["group_same"])                                                # arrays no rule in force reads may be NULL
    got, nall = _build(fx, inp, d_x, d_cls, d_type=0, d_molecule=0)
    _same_list("only d_mask", got, nall, xref.filter_list(ref, cases["group_same"], cls.type, cls.mask, cls.molecule), at)
    null = SimpleNamespace(data_ptr=lambda: 0)
    for kw in (dict(x=null), dict(nlocal=at.nall + 1), dict(nlocal=-1), dict(cutneigh=s.cutoff * (1 - 1e-12)), dict(cutneigh=float("nan")),
               dict(prd_half=(1.0, -1.0, 1.0)), dict(d_tag=d_cls[0].data_ptr())):
        with pytest.raises(ConpError) as e:
            _build(fx, inp, kw.pop("x", d_x), d_cls, **kw)
        assert e.value.code == -1, kw
        with pytest.raises(ConpError) as e:
            fx.pair_get_list()
        assert e.value.code == -2, kw
        valid()
    x = at.x.copy(); x[700, 1] = float("nan")
    with pytest.raises(ConpError) as e:
        _build(fx, inp, _dev(x, np.float64), d_cls)
    assert e.value.code == -4
    valid()
    # a type outside [0, ntypes] is clamped for the look-up: 99 reads row ntypes, -7 row 0
    typ = cls.type.copy()
    typ[cls.type == 5] = 99
    typ[cls.type == 1] = -7
    _set(fx, cases["type_tt"])
    got, nall = _build(fx, inp, d_x, (_dev(typ, np.int32), d_cls[1], d_cls[2]))
    _same_list("clamped types", got, nall, xref.filter_list(ref, cases["type_tt"], cls.type, cls.mask, cls.molecule), at)
    fx.close()


# ---- the zmirror deck's box: the fix re-neighboured on the device behind an excluded build --------------------------------------------
SOLNEG, SOLPOS = 2, 4          # the deck's groups `solneg` and `solpos` as bit masks (bit 0: all)


@functools.lru_cache(maxsize=None)
def zmirror_box():
    """systems.deck("il_onelayer", "zmirror") with the deck's groups and its rule `neigh_modify exclude group solpos solpos`, and the
    host arrays of the setup at x0: atoms with ghosts and the plain half list, built on the device by a scratch handle"""
    import test_gpu_post_neighbor_device as tpn
    import ghost_ref as gref
    s = dataclasses.replace(systems.deck("il_onelayer", "zmirror", etypes=False), newton=False, eletypes=None)
    n = s.natoms
    sol, pos = s.echeck == 0, s.x[:, 2] >= 0.0
    mask = np.ones(n, np.int32)
    mask[sol & pos] |= SOLPOS
    mask[sol & ~pos] |= SOLNEG
    own = SimpleNamespace(x=s.x.copy(), q=s.q.copy(), type=s.type.copy(), tag=s.tag.copy(), echeck=s.echeck.copy(), mask=mask,
                          molecule=((s.tag.astype(np.int64) - 1) // 3 + 1).astype(np.int32))
    boxlo, boxhi, periodic, cut = gref.box_of(s)
    c = SimpleNamespace(s=s, n=n, own=own, box=(boxlo, boxhi, periodic, cut), cutneigh=cut, newton=False,
                        prd_half=np.where(np.asarray(periodic), 0.5 * (boxhi - boxlo), 0.0),
                        rule=xref.rules(group_pairs=[(SOLPOS, SOLPOS)]))
    fx = FixConp(s)
    tpn._params(fx, s)
    b = tpn._build(fx, c, own.x, wrap=False)
    lst, nall = fx.pair_get_list()
    owner = fx.ghost_get()[2]
    c.at0 = tpn._atoms(c, tpn._host(b.d_x)[:nall], tpn._host(b.d_q)[:nall], owner)
    c.lst0 = lst
    fx.close()
    return c


def zmirror_handle(c, style="conp", potdiff=None):
    """a handle after the host setup at x0 (the setup's list is the plain one: the rule drops no pair with an electrode member)"""
    import test_gpu_post_neighbor_device as tpn
    fx = FixConp(c.s, style=style)
    tpn._params(fx, c.s)
    at0 = dataclasses.replace(c.at0, q=c.at0.q.copy())
    fx.init_lists(c.lst0, c.lst0)
    fx.setup_post_neighbor(at0)
    fx.setup_pre_force(at0, 0, c.s.potdiff if potdiff is None else potdiff)
    fx.pair_set_exclusions(group_pairs=c.rule.group_pairs)
    return fx


def zmirror_reneighbor(fx, c, d_own, wrap=True):
    """the device re-neighbouring sequence of DESIGN.md section 25 on the owned coordinates d_own [n][3] (a device tensor, wrapped in
    place): ghost build -> fill / fill_int (tag, type, mask, molecule) -> excluded build -> conp_fix_post_neighbor_device"""
    import torch
    import test_gpu_post_neighbor_device as tpn
    n = c.n
    boxlo, boxhi, periodic, cut = c.box
    if wrap:
        fx.atoms_wrap_device(d_own.data_ptr(), n, boxlo, boxhi, periodic)
    ng = fx.ghost_build_device(d_own.data_ptr(), n, boxlo, boxhi, periodic, cut)
    nall = n + ng
    d_x = torch.full((nall + 8, 3), np.nan, dtype=torch.float64, device="cuda")
    d_q = torch.full((nall + 8,), np.nan, dtype=torch.float64, device="cuda")
    d_x[:n] = d_own[:n]
    d_q[:n] = torch.from_numpy(np.ascontiguousarray(c.own.q)).cuda()
    ints = {}
    for name in ("tag", "type", "mask", "molecule"):
        t = torch.zeros((nall + 8,), dtype=torch.int32, device="cuda")
        t[:n] = torch.from_numpy(np.ascontiguousarray(getattr(c.own, name), dtype=np.int32)).cuda()
        ints[name] = t
    torch.cuda.synchronize()
    fx.ghost_fill_device(d_x.data_ptr(), d_q.data_ptr())
    for t in ints.values():
        fx.ghost_fill_int_device(t.data_ptr(), 1)
    fx.pair_build_list_exclude_device(d_x.data_ptr(), n, nall, c.cutneigh, d_type=ints["type"].data_ptr(), d_mask=ints["mask"].data_ptr(),
                                      d_molecule=ints["molecule"].data_ptr(), prd_half=c.prd_half)
    fx.post_neighbor_device(d_x.data_ptr(), d_q.data_ptr())
    torch.cuda.synchronize()
    return SimpleNamespace(d_x=d_x, d_q=d_q, ints=ints, n=n, nghost=ng, nall=nall, q0=d_q.clone())


def test_the_fix_reneighbours_on_the_device_behind_an_excluded_build():
    """the il_onelayer zmirror box, the deck's rule (group solpos with solpos): the step tables equal those of a host
    conp_fix_post_neighbor fed the downloaded list, and the charges of the next update are equal -- exactly on this Ewald input, when
    two host-route handles are (tests/test_gpu_post_neighbor_device.py)"""
    import test_gpu_post_neighbor_device as tpn
    c = zmirror_box()
    fd, fh, fh2 = (zmirror_handle(c) for _ in range(3))
    rng = np.random.default_rng(41)
    sol = np.nonzero(c.own.echeck == 0)[0]
    step = rng.uniform(-1.0, 1.0, size=(len(sol), 3))
    step *= rng.uniform(0.0, 1.0, size=(len(sol), 1)) / np.linalg.norm(step, axis=1, keepdims=True)
    x1 = c.own.x.copy()
    x1[sol] += step
    b = zmirror_reneighbor(fd, c, _dev(x1, np.float64))
    got, nall = fd.pair_get_list()
    owner = fd.ghost_get()[2]
    full = np.concatenate([np.arange(c.n), owner]).astype(np.int64)
    plain_fx, _ = _handle(c.s, False)
    plain_fx.pair_build_list_device(b.d_x.data_ptr(), c.n, nall, c.cutneigh, prd_half=c.prd_half)
    plain, _ = plain_fx.pair_get_list()
    plain_fx.close()
    want = xref.filter_list(plain, c.rule, c.own.type[full], c.own.mask[full], c.own.molecule[full])
    print(f"zmirror box: {got.neigh.size} of {plain.neigh.size} pairs listed ({1 - got.neigh.size / plain.neigh.size:.3f} dropped)")
    assert 0 < got.neigh.size < plain.neigh.size
    _same_bytes("zmirror box", got, want)
    i, jraw = pref.pairs_of(got)
    mi, mj = c.own.mask[full][i], c.own.mask[full][jraw & xref.NEIGHMASK]
    assert not np.any(mi & mj & SOLPOS)
    td, idv = fd.step_tables(), tpn._info(fd)
    for f in (fh, fh2):
        tpn.host_route(f, c, fd, b)
    tpn._same_tables("zmirror box: device against host route", td, fh.step_tables())
    tpn._same_tables("zmirror box: info", idv, tpn._info(fh))
    assert td["n_b_pairs"] > 0
    uh, uh2 = tpn._update(fh, b, c.s.potdiff), tpn._update(fh2, b, c.s.potdiff)
    exact = uh.q.tobytes() == uh2.q.tobytes() and uh.eleallq.tobytes() == uh2.eleallq.tobytes() and uh.scalar == uh2.scalar
    if not exact:
        print(f"two host-route handles already differ: the bound {tpn.TOL_Q} of tests/test_gpu_parity.py takes the place of byte identity")
    tpn._same_update("zmirror box: device against host route", tpn._update(fd, b, c.s.potdiff), uh, exact)
    for f in (fd, fh, fh2):
        f.close()
