"""-m gpu: conp_potential_atom_device -- `compute potential/atom` on device arrays.

Systems: the dilute deck (ffield, and slab with qsum on and off), the il_onelayer deck with the eta correction on its electrode
molecules, systems.small_random(ne_side=4, n_elyte=96); each with four zero-charge probes (tests/test_gpu_ewald_potential.py's
_add_probes), one of them exactly on an electrolyte atom: the rsq floor.  Each with newton on and off, with the pair list uploaded
(conp_pair_set_list, ghosts folded in numpy) and with list and ghosts built on the device (conp_ghost_build_device ->
conp_pair_build_list_device -> conp_fix_post_neighbor_device, flags' ghost rows by conp_ghost_fill_int_device, conp_ghost_fold_device).

Bounds (the project's own): the pair part within 1e-12 A_a of the longdouble reference of tests/potential_ref.py, A_a = sum |q_b
dudq| (the bound style of tests/test_gpu_pair_forces.py); the full result after the fold within 1e-11 max|pot| of
conp_compute_potential_atom on the selected owned rows (tests/test_gpu_ewald_potential.py:83,101) -- the maximum is taken WITHOUT
the probe that sits on an atom, whose 1e5 V would make the bound say nothing about the other rows; the electrode's flatness within
1e-8 dv (:146-150); the pppm handle against the oracle within 1e-10 (tests/test_gpu_pppm.py:178)."""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import ghost_ref as gref
import pair_force_ref as pref
import potential_ref as pr
import transpose_ref as tr
from conp_amd import ConpError, FixConp, capi, neighbor, systems
from helpers import rel_err

pytestmark = pytest.mark.gpu
EVS = systems.QQR2E / systems.QE2F
TOL_PAIR, TOL_FULL, TOL_FLAT, TOL_ORACLE = 1e-12, 1e-11, 1e-8, 1e-10
DV = 1.7
NAN = float("nan")
SYSTEMS = [("dilute", "ffield"), ("dilute", "slab"), ("il_onelayer", "ffield"), ("small", "ffield")]
ROUTES = [(False, False), (False, True), (True, False), (True, True)]      # (newton, built)
PPPM_CASES = [("dilute", "ffield", (27, 24, 144), 0.0), ("dilute", "slab", (27, 24, 432), 1.979), ("il_onelayer", "ffield", (36, 40, 150), 1.979)]


def _dev(a, dtype=np.float64):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()
    torch.cuda.synchronize()
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


@functools.lru_cache(maxsize=None)
def system(name, mode, newton, probes=True):
    s = systems.small_random(ne_side=4, n_elyte=96, mode=mode) if name == "small" else systems.deck(name, mode, etypes=False)
    s = dataclasses.replace(s, newton=newton, eletypes=None)
    if not probes:
        return s, np.zeros(0, np.int64)
    el = np.nonzero((s.echeck == 0) & (s.q != 0))[0]
    q, x = s.q.copy(), s.x.copy()
    centre = s.boxlo + 0.5 * np.asarray(s.prd)
    for k, i in enumerate(el[:4]):
        q[i] = 0.0
        x[i] = centre + np.array([0.37 * k, -0.21 * k, 0.53 * k - 0.8])
    x[el[3]] = x[el[9]]                                             # exactly on a charged electrolyte atom
    return dataclasses.replace(s, q=q, x=x), el[:4]


@functools.lru_cache(maxsize=None)
def case(name, mode, newton, built, probes=True, mesh=None):
    """a handle with solved electrode charges that holds the pair list and its transposed index, the device arrays of its atoms and
    their host copies: formed once per process and shared (the entry keeps nothing between calls but the reuse bit)"""
    import torch
    s, pb = system(name, mode, newton, probes)
    n = s.natoms
    at0, lst0, _ = neighbor.build_lists(s)
    kw = dict(extra_args=["pppm"], pppm_mesh=mesh[0], pppm_order=mesh[1]) if mesh else {}
    fx = FixConp(s, **kw)
    p = pref.lj_tables(s.ntypes, s.cutoff)
    fx.pair_set_params(p.cutsq, p.cut_coul, p.lj)
    fx.init_lists(lst0, lst0)
    fx.setup_post_neighbor(at0)
    fx.setup_pre_force(at0, 0, DV)                                  # at0.q: the electrode atoms carry their solved charges
    if not built:
        fx.pre_force(at0, 1, DV)
        fx.pair_set_list(lst0, at0.nall)
        at, lst = at0, lst0
        d_x, d_q = _dev(at.x), _dev(at.q)
    else:
        boxlo, boxhi, periodic, cut = gref.box_of(s)
        d_own = _dev(s.x)
        ng = fx.ghost_build_device(d_own.data_ptr(), n, boxlo, boxhi, periodic, cut)
        nall = n + ng
        d_x = torch.full((nall, 3), NAN, dtype=torch.float64, device="cuda")
        d_q = torch.full((nall,), NAN, dtype=torch.float64, device="cuda")
        d_x[:n] = d_own
        d_q[:n] = _dev(at0.q[:n])
        torch.cuda.synchronize()
        fx.ghost_fill_device(d_x.data_ptr(), d_q.data_ptr())
        fx.pair_build_list_device(d_x.data_ptr(), n, nall, cut, prd_half=np.where(np.asarray(periodic), 0.5 * np.asarray(s.prd), 0.0))
        fx.post_neighbor_device(d_x.data_ptr(), d_q.data_ptr())
        fx.pre_force_device(d_x.data_ptr(), d_q.data_ptr(), DV)
        fx.ghost_fill_device(d_x.data_ptr(), d_q.data_ptr())        # the ghosts' charges follow the update's
        lst, nall_ = fx.pair_get_list()
        _, ng_, owner, _ = fx.ghost_get()
        assert nall_ == nall and ng_ == ng
        full = np.concatenate([np.arange(n), owner]).astype(np.int64)
        at = neighbor.Atoms(nlocal=n, nghost=ng, x=_host(d_x).copy(), q=_host(d_q).copy(), type=s.type[full].copy(), tag=s.tag[full].copy(),
                            echeck=s.echeck[full].copy(), owner=full.astype(np.int32))
    fx.pair_transpose_list_device()
    return SimpleNamespace(s=s, fx=fx, at=at, lst=lst, n=n, nall=at.nall, ntotal=at.nall if newton else n, newton=newton, built=built,
                           probes=pb, d_x=d_x, d_q=d_q, owner=np.asarray(at.owner, np.int64), mesh=mesh,
                           cutsq=s.cutsq_table(), cut_coulsq=pr.cut_coulsq_of(s.cutoff, s.g_ewald),
                           eta=s.eta if name == "il_onelayer" else 0.0, etasel=(at.echeck != 0).astype(np.int32),
                           tag=f"{name} {mode}, newton {'on' if newton else 'off'}, list {'built' if built else 'uploaded'}")


def flags_on_device(c, flags):
    """[nall] int32 on the device; on the built route the ghost rows come from conp_ghost_fill_int_device, as the header says"""
    import torch
    if not c.built:
        return _dev(flags, np.int32)
    d = torch.full((c.nall,), -1, dtype=torch.int32, device="cuda")
    d[:c.n] = _dev(flags[:c.n], np.int32)
    torch.cuda.synchronize()
    c.fx.ghost_fill_int_device(d.data_ptr(), 1)
    return d


def run(c, sel_owned, eta=None, fold=True, fill=NAN, times=1, d_x=None, d_q=None, **kw):
    """the entry on selection sel_owned [nlocal] (ghost rows follow their owners) -> list of d_pot [nall + 8] as numpy, folded if asked"""
    import torch
    eta = c.eta if eta is None else eta
    sel = np.asarray(sel_owned)[c.owner]
    flags, targets, nt = capi.potential_selection(sel, c.etasel if eta != 0.0 else None, c.n)
    d_flags, d_targets = flags_on_device(c, flags), _dev(targets, np.int32)
    if c.built:
        assert np.array_equal(_host(d_flags), flags)
    X, Q = (c.d_x if d_x is None else d_x), (c.d_q if d_q is None else d_q)
    outs = []
    for _ in range(times):
        d_pot = torch.full((c.nall + 8,), fill, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        c.fx.potential_atom_device(X.data_ptr(), Q.data_ptr(), d_flags.data_ptr(), nt, d_targets.data_ptr(), d_pot.data_ptr(), eta=eta, **kw)
        if fold and c.newton and c.built:
            c.fx.ghost_fold_device(d_pot.data_ptr(), 1)
        outs.append(d_pot)
    out = [_host(t).copy() for t in outs]
    if fold and c.newton and not c.built:
        for o in out:
            o[:c.n] = pr.fold(o[:c.nall], c.owner, c.n)
    return out


@functools.lru_cache(maxsize=None)
def listed_pairs(c_key):
    """(i, j, dudq) of the case's listed pairs inside the cutoffs, in longdouble: formed once per case, shared by every selection"""
    c = case(*c_key)
    flags = (c.etasel << 1) if c.eta != 0.0 else np.zeros(c.nall, np.int32)
    return pr._pairs(np.asarray(c.at.x, pr.LD), np.asarray(c.at.q, pr.LD), c.at.type, flags, c.lst, c.cutsq, c.cut_coulsq, c.s.g_ewald, c.eta)


def pair_reference(c_key, sel_owned):
    """pr.pair_loop on the shared pairs -> (pot, A) [nall] in e / A"""
    c = case(*c_key)
    i, j, dudq = listed_pairs(c_key)
    q = np.asarray(c.at.q, pr.LD)
    sel = np.asarray(sel_owned)[c.owner] != 0
    gate = (sel[i] | sel[j]) & ((q[i] != 0) | (q[j] != 0)) & (c.newton | sel[i] | (j < c.n))
    i, j, dudq = i[gate], j[gate], dudq[gate]
    pot, A = np.zeros(c.nall, pr.LD), np.zeros(c.nall, pr.LD)
    mine, recv = sel[i], (j < c.n) | c.newton
    np.add.at(pot, i[mine], (q[j] * dudq)[mine]); np.add.at(A, i[mine], np.abs(q[j] * dudq)[mine])
    np.add.at(pot, j[recv], (q[i] * dudq)[recv]); np.add.at(A, j[recv], np.abs(q[i] * dudq)[recv])
    return pot, A


def selections(c):
    n = c.n
    rng = np.random.default_rng(11)
    half = (rng.random(n) < 0.5).astype(np.int32)
    half[c.probes] = 1
    half[np.nonzero(c.at.echeck[:n] != 0)[0][:7]] = 1
    one, probe = np.zeros(n, np.int32), np.zeros(n, np.int32)
    one[np.nonzero(c.at.echeck[:n] != 0)[0][3]] = 1
    probe[c.probes[3]] = 1                                          # the probe on an atom, alone
    return dict(none=np.zeros(n, np.int32), one=one, probe=probe, half=half, all=np.ones(n, np.int32))


def check_rows(c, got, sel_owned, tag):
    """unselected rows of [0, ntotal) exactly 0, rows from ntotal on keep the NaN pre-fill"""
    sel = np.asarray(sel_owned)[c.owner] != 0
    assert np.all(got[:c.ntotal][~sel[:c.ntotal]] == 0.0), tag
    assert not np.isnan(got[:c.ntotal]).any(), tag
    assert np.all(np.isnan(got[c.ntotal:])), tag


def host_entry(c, sel_owned, **kw):
    """conp_compute_potential_atom at the case's host arrays and list, ghost rows folded onto their owners -> [nlocal]"""
    sel = np.asarray(sel_owned, np.int32)[c.owner]
    pot = c.fx.compute_potential_atom(c.at, c.lst, sel, c.etasel if kw.get("eta", 0.0) != 0.0 else None, **kw)
    return pr.fold(pot[:c.ntotal], c.owner, c.n) if c.newton else pot[:c.n]


def full_scale(c, want, rows):
    """max |pot| over the selected owned rows without the probe on an atom (see the module docstring), unless it is alone"""
    others = rows[rows != c.probes[3]] if len(c.probes) else rows
    rows = others if len(others) else rows
    return np.abs(want[rows]).max() if len(rows) else 0.0


# ---- accuracy, every system, route and selection ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("newton,built", ROUTES)
@pytest.mark.parametrize("name,mode", SYSTEMS)
def test_pair_part_and_full_result(name, mode, newton, built):
    key = (name, mode, newton, built)
    c = case(*key)
    if c.eta != 0.0:                                                # 0, 1 and 2 eta members among the listed pairs
        i, j, _ = listed_pairs(key)
        assert {0, 1, 2} == set(np.unique(c.etasel[i] + c.etasel[j]))
    i, jraw = pref.pairs_of(c.lst)
    d = c.at.x[i] - c.at.x[jraw & pref.NEIGHMASK]
    assert ((d * d).sum(axis=1) < 1e-10).sum() >= 1                 # the rsq floor is met
    for sname, sel in selections(c).items():
        tag = f"{c.tag}, selection {sname}"
        rows = np.nonzero(sel)[0]
        # pair only, not folded: every row of [0, ntotal) against its own partial sum
        got = run(c, sel, fold=False, pair=True, kspace=False)[0]
        check_rows(c, got, sel, tag)
        ref, A = pair_reference(key, sel)
        selall = np.nonzero(sel[c.owner][:c.ntotal])[0]
        err = np.abs(got[:c.nall].astype(pr.LD) - ref * pr.LD(EVS))[selall]
        bound = TOL_PAIR * A[selall] * pr.LD(EVS)
        assert np.all(err[bound == 0] == 0), tag
        fr = float((err[bound > 0] / bound[bound > 0]).max()) if np.any(bound > 0) else 0.0
        print(f"{tag}: pair part {fr:.3g} of the bound 1e-12 A")
        assert fr <= 1.0, (tag, fr)
        # the full result after the fold against the host entry, qsum on and (slab) off
        for qsum in ((True, False) if c.s.slabflag else (True,)):
            got = run(c, sel, pair=True, kspace=True, qsum=qsum)[0]
            check_rows(c, got, sel, tag)
            want = host_entry(c, sel, eta=c.eta, pair=True, kspace=True, qsum=qsum)
            scale = full_scale(c, want, rows)
            e = np.abs(got[rows] - want[rows]).max() if len(rows) else 0.0
            print(f"{tag}, qsum {qsum}: full result |dev - host| {e:.3e}, max|pot| {scale:.3e}")
            assert e <= TOL_FULL * scale, (tag, qsum, e, scale)
        # k-space only
        got = run(c, sel, pair=False, kspace=True)[0]
        check_rows(c, got, sel, tag)
        want = host_entry(c, sel, eta=c.eta, pair=False, kspace=True)
        if len(rows):
            assert np.abs(got[rows] - want[rows]).max() <= TOL_FULL * np.abs(want[rows]).max(), tag
            assert np.all(got[c.n:c.ntotal] == 0.0)                 # no k-space part on ghost rows
    if name == "dilute" and mode == "slab":                         # the two slab terms act
        a, b = run(c, selections(c)["all"], qsum=True)[0][:c.n], run(c, selections(c)["all"], qsum=False)[0][:c.n]
        assert np.abs(a - b).max() > 1e-6 * np.abs(a).max()


@pytest.mark.parametrize("count", [1, 63, 64, 65, 129])
def test_target_counts_at_the_block_edges(count):
    """the block edges of tests/test_gpu_ewald_shapes.py; with blocks of 64 targets, 65 and 129 take two and three blocks"""
    c = case("dilute", "ffield", True, True)
    rng = np.random.default_rng(count)
    sel = np.zeros(c.n, np.int32)
    sel[rng.choice(c.n, count, replace=False)] = 1
    want = host_entry(c, sel, eta=0.0)
    rows = np.nonzero(sel)[0]
    for width in (0, 64):
        capi.set_ew_block(width)
        try:
            got = run(c, sel)[0]
        finally:
            capi.set_ew_block(0)
        check_rows(c, got, sel, f"{count} targets")
        assert np.abs(got[rows] - want[rows]).max() <= TOL_FULL * full_scale(c, want, rows), (count, width)


# ---- the crafted list -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("newton", [False, True])
def test_the_crafted_list_with_real_coordinates(newton):
    """rows and transposed segments of 0, 1, 63, 64, 65 and 129 entries, a row that is empty while its segment is not; entries with
    special bits give the bytes of the same list with the bits cleared"""
    c = case("small", "ffield", newton, False)
    assert c.nall >= tr.N_OWN + tr.N_TARGET + 40
    lst = tr.crafted_list(c.nall, targets=tr.central_targets(c.at.x, c.n))
    rows, segs = tr.segment_lengths(lst, c.nall)
    for k in (0, 1, 63, 64, 65, 129):
        assert np.any(rows == k) and np.any(segs == k)
    assert np.any((rows == 0) & (segs > 0))
    bare = dataclasses.replace(lst, neigh=(lst.neigh & pref.NEIGHMASK).astype(np.int32))
    assert np.any(bare.neigh != lst.neigh)
    sel = np.ones(c.n, np.int32)
    flags = np.ones(c.nall, np.int32)
    outs = []
    try:
        for L in (lst, bare):
            c.fx.pair_set_list(L, c.nall)
            c.fx.pair_transpose_list_device()
            outs.append(run(c, sel, eta=0.0, fold=False, pair=True, kspace=False)[0])
    finally:
        c.fx.pair_set_list(c.lst, c.nall)
        c.fx.pair_transpose_list_device()
    assert outs[0].tobytes() == outs[1].tobytes()
    check_rows(c, outs[0], sel, "crafted list")
    ref, A = pr.pair_loop(c.at.x, c.at.q, c.at.type, flags, c.n, lst, c.cutsq, c.cut_coulsq, c.s.g_ewald, 0.0, newton)
    err = np.abs(outs[0][:c.ntotal].astype(pr.LD) - ref[:c.ntotal] * pr.LD(EVS))
    bound = TOL_PAIR * A[:c.ntotal] * pr.LD(EVS)
    assert np.all(err[bound == 0] == 0) and np.count_nonzero(bound) > c.n // 2
    assert float((err[bound > 0] / bound[bound > 0]).max()) <= 1.0


# ---- the self-check of the package ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [("dilute", "slab"), ("dilute", "ffield"), ("il_onelayer", "ffield")])
def test_electrode_atoms_sit_at_the_applied_potential(name, mode):
    """with the eta correction every electrode atom sits at its applied potential (the assertions of
    tests/test_gpu_ewald_potential.py:146-150), from the device-built pair list and the device update's charges"""
    c = case(name, mode, True, True, probes=False)
    s, n = c.s, c.n
    pot = run(c, np.ones(n, np.int32), eta=s.eta)[0][:n]
    ec = c.at.echeck[:n]
    if mode == "ffield":
        z = c.at.x[:n, 2]
        zhalf = s.boxlo[2] + 0.5 * s.prd[2]
        d = np.where((ec == 1) & (z < zhalf), -(z / s.prd[2] + 1.0), -z / s.prd[2])
        resid = pot[ec != 0] - DV * d[ec != 0]
        assert resid.max() - resid.min() <= TOL_FLAT * DV, resid.max() - resid.min()
    else:
        left, right = pot[ec == 1], pot[ec == -1]
        assert left.max() - left.min() <= TOL_FLAT * DV and right.max() - right.min() <= TOL_FLAT * DV, (np.ptp(left), np.ptp(right))
        assert abs((right.mean() - left.mean()) - DV) <= TOL_FLAT * DV, right.mean() - left.mean()


# ---- determinism ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("newton", [False, True])
def test_three_calls_on_two_fresh_handles_are_byte_identical(newton):
    outs = []
    for _ in range(2):
        c = case.__wrapped__("small", "ffield", newton, True)        # (not the shared handle: a fresh one)
        outs += run(c, selections(c)["half"], eta=c.s.eta, times=3)
        c.fx.close()
    assert not np.isnan(outs[0][:c.ntotal]).any() and np.abs(outs[0][:c.n]).max() > 0
    for o in outs[1:]:
        assert o.tobytes() == outs[0].tobytes()                     # every row, ghost rows and the NaN tail included


def test_pair_part_on_a_pppm_handle_is_byte_identical():
    """the mesh update spreads with float atomics, so two pppm handles solve charges that differ in their last bits: both handles
    are given the FIRST handle's x and q, and the pair part of those is the same bytes on both"""
    outs, xq = [], None
    for _ in range(2):
        c = case.__wrapped__("dilute", "ffield", True, True, True, ((27, 24, 144), 5))
        xq = (c.at.x.copy(), c.at.q.copy()) if xq is None else xq
        assert xq[0].tobytes() == c.at.x.tobytes()                  # (the same ghosts in the same order)
        outs += run(c, selections(c)["half"], times=3, fold=False, pair=True, kspace=False, d_x=_dev(xq[0]), d_q=_dev(xq[1]))
        c.fx.close()
    assert np.abs(outs[0][:c.nall]).max() > 0
    for o in outs[1:]:
        assert o.tobytes() == outs[0].tobytes()


# ---- reuse ---------------------------------------------------------------------------------------------------------------------------------
def _forces(c, f_pre):
    """the device k-space force entry on a copy of f_pre -> (f, eatom) as numpy"""
    import torch
    d_f = _dev(f_pre)
    d_e = torch.full((c.n,), NAN, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    (c.fx.pppm_forces_device if c.mesh else c.fx.ewald_forces_device)(c.d_x.data_ptr(), c.d_q.data_ptr(), d_f.data_ptr(), 0, d_e.data_ptr())
    return _host(d_f).copy(), _host(d_e).copy()


@pytest.mark.parametrize("name,mode", [("dilute", "slab"), ("il_onelayer", "ffield")])
def test_reuse_after_the_ewald_force_entry_is_byte_identical(name, mode):
    c = case(name, mode, True, True)
    sel = selections(c)["half"]
    f_pre = np.random.default_rng(5).normal(size=(c.nall, 3))
    plain = run(c, sel, reuse_kspace=False)[0]
    f0, e0 = _forces(c, f_pre)
    again = run(c, sel, reuse_kspace=True, times=2)
    assert plain.tobytes() == again[0].tobytes() == again[1].tobytes()
    # the force entry after a potential call, reusing or not, returns the bytes it returned before
    f1, e1 = _forces(c, f_pre)
    run(c, sel, reuse_kspace=False)
    f2, e2 = _forces(c, f_pre)
    assert f0.tobytes() == f1.tobytes() == f2.tobytes() and e0.tobytes() == e1.tobytes() == e2.tobytes()


def test_reuse_on_a_pppm_handle_agrees_to_the_spread_s_rounding():
    c = case.__wrapped__("dilute", "slab", True, True, True, ((27, 24, 432), 5))
    sel = selections(c)["half"]
    rows = np.nonzero(sel)[0]
    plain = run(c, sel, reuse_kspace=False)[0]
    want = host_entry(c, sel, eta=0.0)
    assert np.abs(plain[rows] - want[rows]).max() <= TOL_FULL * full_scale(c, want, rows)
    _forces(c, np.zeros((c.nall, 3)))
    again = run(c, sel, reuse_kspace=True)[0]
    assert np.abs(plain[rows] - again[rows]).max() <= TOL_FULL * full_scale(c, plain, rows)
    # the brick is left only by a call that asked for d_f or d_eatom
    import torch
    d_ev = torch.zeros(8, dtype=torch.float64, device="cuda")
    c.fx.pppm_forces_device(c.d_x.data_ptr(), c.d_q.data_ptr(), 0, d_ev.data_ptr(), 0)
    with pytest.raises(ConpError) as e:
        run(c, sel, reuse_kspace=True)
    assert e.value.code == -2 and "reuse_kspace" in str(e.value)                  # CONP_ERR_STATE
    c.fx.close()


def _refused_untouched(c, sel, what):
    """a reuse call without a valid bit: CONP_ERR_STATE, d_pot keeps its bytes"""
    import torch
    flags, targets, nt = capi.potential_selection(np.asarray(sel)[c.owner], None, c.n)
    d_flags, d_targets = _dev(flags, np.int32), _dev(targets, np.int32)
    pre = np.random.default_rng(2).normal(size=c.nall + 8)
    d_pot = _dev(pre)
    with pytest.raises(ConpError) as e:
        c.fx.potential_atom_device(c.d_x.data_ptr(), c.d_q.data_ptr(), d_flags.data_ptr(), nt, d_targets.data_ptr(), d_pot.data_ptr(),
                                   reuse_kspace=True)
    assert e.value.code == -2 and "reuse_kspace" in str(e.value), what          # CONP_ERR_STATE
    assert _host(d_pot).tobytes() == pre.tobytes(), what


def test_reuse_without_a_valid_bit_is_refused():
    c = case.__wrapped__("dilute", "ffield", True, True)
    sel = selections(c)["half"]
    _refused_untouched(c, sel, "fresh handle")                      # (no device force entry was called on it yet)
    _forces(c, np.zeros((c.nall, 3)))
    run(c, sel, reuse_kspace=True)
    c.fx.pre_force_device(c.d_x.data_ptr(), c.d_q.data_ptr(), DV)
    _refused_untouched(c, sel, "after conp_fix_pre_force_device")
    _forces(c, np.zeros((c.nall, 3)))
    c.fx.post_neighbor_device(c.d_x.data_ptr(), c.d_q.data_ptr())
    _refused_untouched(c, sel, "after a device re-neighbouring")
    c.fx.pre_force_device(c.d_x.data_ptr(), c.d_q.data_ptr(), DV)
    _forces(c, np.zeros((c.nall, 3)))
    c.fx.ewald_compute(c.at)
    _refused_untouched(c, sel, "after a host query entry")
    _forces(c, np.zeros((c.nall, 3)))
    run(c, sel, reuse_kspace=False)
    _refused_untouched(c, sel, "after a call without reuse")
    _forces(c, np.zeros((c.nall, 3)))
    run(c, sel, reuse_kspace=True)                                  # ... and valid again
    c.fx.close()


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def test_refusals():
    import torch
    c = case("small", "ffield", True, False)
    fx = c.fx
    sel = selections(c)["half"]
    flags, targets, nt = capi.potential_selection(sel[c.owner], c.etasel, c.n)
    F, T = _dev(flags, np.int32), _dev(targets, np.int32)
    pre = np.random.default_rng(3).normal(size=c.nall + 8)
    d_pot = _dev(pre)
    X, Q, P = c.d_x.data_ptr(), c.d_q.data_ptr(), d_pot.data_ptr()

    def refused(code, *a, **k):
        with pytest.raises(ConpError) as e:
            fx.potential_atom_device(*a, **k)
        assert e.value.code == code, (a, k, str(e.value))
        assert _host(d_pot).tobytes() == pre.tobytes()
    ARG, STATE = -1, -2
    lib = capi.load_library()
    import ctypes as C
    pa = capi.conp_potential_args(pairflag=1, kspaceflag=1, qsumflag=1, eta=0.0)
    vp = C.c_void_p
    assert lib.conp_potential_atom_device(None, vp(X), vp(Q), vp(F.data_ptr()), nt, vp(T.data_ptr()), C.byref(pa), 0, vp(P)) == ARG
    assert lib.conp_potential_atom_device(fx.h, vp(X), vp(Q), vp(F.data_ptr()), nt, vp(T.data_ptr()), None, 0, vp(P)) == ARG
    refused(ARG, 0, Q, F.data_ptr(), nt, T.data_ptr(), P)
    refused(ARG, X, 0, F.data_ptr(), nt, T.data_ptr(), P)
    refused(ARG, X, Q, F.data_ptr(), -1, T.data_ptr(), P)
    refused(ARG, X, Q, F.data_ptr(), c.n + 1, T.data_ptr(), P)
    refused(ARG, X, Q, F.data_ptr(), nt, 0, P)
    refused(ARG, X, Q, 0, nt, T.data_ptr(), P)                      # the pair part needs d_flags
    refused(ARG, X, Q, 0, nt, T.data_ptr(), P, pair=False, eta=1.0)  # so does eta
    # NULL d_flags is fine for the k-space part alone; NULL d_pot: CONP_OK, nothing done; ntargets 0 with NULL d_targets
    fx.potential_atom_device(X, Q, 0, nt, T.data_ptr(), P, pair=False)
    got = _host(d_pot).copy()
    want = host_entry(c, sel, eta=0.0, pair=False, kspace=True)
    rows = np.nonzero(sel)[0]
    assert np.abs(got[rows] - want[rows]).max() <= TOL_FULL * np.abs(want[rows]).max()
    assert got[c.ntotal:].tobytes() == pre[c.ntotal:].tobytes()
    fx.potential_atom_device(X, Q, F.data_ptr(), nt, T.data_ptr(), 0)
    fx.potential_atom_device(X, Q, F.data_ptr(), 0, 0, P, pair=False)
    # both flags zero: [0, ntotal) is zeroed, the rows behind keep their bytes
    d_pot.copy_(_dev(pre))
    fx.potential_atom_device(X, Q, F.data_ptr(), nt, T.data_ptr(), P, pair=False, kspace=False)
    got = _host(d_pot)
    assert np.all(got[:c.ntotal] == 0.0) and got[c.ntotal:].tobytes() == pre[c.ntotal:].tobytes()
    d_pot.copy_(_dev(pre))
    torch.cuda.synchronize()
    # the pair list: an index of an earlier list, then none at all
    fx.pair_set_list(c.lst, c.nall)
    refused(STATE, X, Q, F.data_ptr(), nt, T.data_ptr(), P)
    fx.potential_atom_device(X, Q, F.data_ptr(), nt, T.data_ptr(), P, pair=False)      # (the k-space part alone needs no list)
    d_pot.copy_(_dev(pre))
    torch.cuda.synchronize()
    fx.pair_transpose_list_device()
    # before (setup_)post_neighbor; a pppm-less handle and a handle without a pair list
    s = c.s
    f2 = FixConp(s)
    try:
        with pytest.raises(ConpError) as e:
            f2.potential_atom_device(X, Q, F.data_ptr(), nt, T.data_ptr(), P)
        assert e.value.code == STATE
        f2.init_lists(c.lst, c.lst)
        f2.setup_post_neighbor(c.at)
        with pytest.raises(ConpError) as e:
            f2.potential_atom_device(X, Q, F.data_ptr(), nt, T.data_ptr(), P)
        assert e.value.code == STATE and "list" in str(e.value)
    finally:
        f2.close()
    assert _host(d_pot).tobytes() == pre.tobytes()


# ---- the pppm handle against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("deck,mode,mesh,eta", PPPM_CASES)
def test_pppm_handle_matches_the_oracle(oracle, deck, mode, mesh, eta):
    """the cases and flag combinations of tests/test_gpu_pppm.py:158-178 through the device entry"""
    import torch
    import oracle_py
    from test_gpu_pppm import _pppm_handle
    order = 5 if mesh[0] != 36 else 4
    s, at, alist, blist, fx = _pppm_handle(deck, mode, mesh, order)
    s_gen = systems.deck(deck, mode, etypes=False)
    at_g, plist, _ = neighbor.build_lists(s_gen)
    assert at_g.nlocal == at.nlocal and np.array_equal(at_g.tag, at.tag)
    n, nall = at.nlocal, at.nlocal + at.nghost
    assert not s.newton
    rng = np.random.default_rng(8)
    sel = (rng.random(nall) < 0.5).astype(np.int32)
    sel[n:] = sel[at.owner[n:]]
    etasel = (at.echeck != 0).astype(np.int32)
    fx.pair_set_list(plist, nall)
    fx.pair_transpose_list_device()
    flags, targets, nt = capi.potential_selection(sel, etasel, n)
    d_x, d_q, F, T = _dev(at.x), _dev(at.q), _dev(flags, np.int32), _dev(targets, np.int32)
    pp = oracle_py.Pppm(oracle, s, mesh, order)
    own = np.nonzero(sel[:n])[0]
    for kw in (dict(pair=True, kspace=True, qsum=True), dict(pair=True, kspace=False, qsum=True), dict(pair=False, kspace=True, qsum=False)):
        d_pot = torch.full((nall,), NAN, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        fx.potential_atom_device(d_x.data_ptr(), d_q.data_ptr(), F.data_ptr(), nt, T.data_ptr(), d_pot.data_ptr(), eta=eta, **kw)
        got = _host(d_pot)
        want = pp.compute_potential_atom(s, at, plist, sel, etasel, eta=eta, **kw)
        assert np.abs(want[own]).max() > 0
        assert rel_err(got[own], want[own]) < TOL_ORACLE, kw
        assert np.all(got[:n][sel[:n] == 0] == 0.0) and np.all(np.isnan(got[n:]))
    pp.close(); fx.close()
