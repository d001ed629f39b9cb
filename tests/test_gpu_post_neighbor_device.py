"""-m gpu: conp_fix_post_neighbor_device -- the fix re-neighboured from the handle's own half list and ghost
map and the device arrays of the call -- against the host route on the identical list, and against the numpy restatement of
tests/post_neighbor_ref.py.

Every case: handles with the same host setup at x0; the owned atoms move (tests/post_neighbor_ref.py::case); handle D runs wrap ->
ghost build -> fill -> list build -> conp_fix_post_neighbor_device -> conp_fix_pre_force_device; handle H gets D's list and ghosts
(conp_pair_get_list, conp_ghost_get) and the host copies of D's filled arrays through conp_fix_init_list + conp_fix_post_neighbor, and
runs conp_fix_pre_force_device on the same device arrays.  (1) every array of conp_fix_get_step_tables, the sizes and conp_info's
z-window / list figures are equal between D, H and the reference;  (2) the charges and the fix scalar of D and H are byte-identical
-- after two H-route handles were found byte-identical to each other (where they are not, the bound of tests/test_gpu_parity.py,
1e-8 of the largest charge, takes the place of byte identity, and the test says so)."""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import pair_force_ref as pref
import post_neighbor_ref as pnr
from conp_amd import ConpError, FixConp, capi, neighbor

pytestmark = pytest.mark.gpu

PPPM = dict(extra_args=["pppm"], pppm_mesh=(27, 24, 144), pppm_order=5)
TOL_Q = 1e-8              # tests/test_gpu_parity.py: charges, relative to the largest entry


def _dev(a, dtype):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()
    torch.cuda.synchronize()
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _params(fx, s, scale=1.0):
    p = pref.lj_tables(s.ntypes, s.cutoff * scale)
    fx.pair_set_params(p.cutsq, p.cut_coul, p.lj)


def _build(fx, c, x_owned, wrap=True, nlocal=None, with_ghosts=True):
    """wrap -> ghost build -> fill (+ tag) -> list build on the owned coordinates given: the device arrays and sizes"""
    import torch
    n = c.n if nlocal is None else nlocal
    boxlo, boxhi, periodic, cut = c.box
    d_own = _dev(x_owned[:n], np.float64)
    if wrap:
        fx.atoms_wrap_device(d_own.data_ptr(), n, boxlo, boxhi, periodic)
    ng = fx.ghost_build_device(d_own.data_ptr(), n, boxlo, boxhi, periodic, cut)
    nall = n + ng
    d_x = torch.full((nall + 8, 3), np.nan, dtype=torch.float64, device="cuda")
    d_q = torch.full((nall + 8,), np.nan, dtype=torch.float64, device="cuda")
    d_tag = torch.zeros((nall + 8,), dtype=torch.int32, device="cuda")
    d_x[:n] = d_own
    d_q[:n] = torch.from_numpy(np.ascontiguousarray(c.own.q[:n])).cuda()
    d_tag[:n] = torch.from_numpy(np.ascontiguousarray(c.own.tag[:n])).cuda()
    torch.cuda.synchronize()
    fx.ghost_fill_device(d_x.data_ptr(), d_q.data_ptr())
    fx.ghost_fill_int_device(d_tag.data_ptr(), 1)
    fx.pair_build_list_device(d_x.data_ptr(), n, nall if with_ghosts else n, c.cutneigh, prd_half=c.prd_half)
    torch.cuda.synchronize()
    return SimpleNamespace(d_x=d_x, d_q=d_q, d_tag=d_tag, n=n, nghost=ng, nall=nall, q0=d_q.clone())


def _atoms(c, x_all, q_all, owner):
    full = np.concatenate([np.arange(c.n), owner]).astype(np.int64)
    return neighbor.Atoms(nlocal=c.n, nghost=len(owner), x=np.ascontiguousarray(x_all), q=np.ascontiguousarray(q_all),
                          type=c.own.type[full].copy(), tag=c.own.tag[full].copy(), echeck=c.own.echeck[full].copy(),
                          owner=full.astype(np.int32))


@functools.lru_cache(maxsize=None)
def setup_inputs(kind, newton):
    """the host arrays of the setup at x0, formed once per case: atoms with ghosts (the reference's map) and the half list, which a
    scratch handle builds on the device (the build is tested by tests/test_gpu_pair_build_list.py)"""
    c = pnr.case(kind, newton)
    fx = FixConp(c.s, **(PPPM if kind == "il_onelayer" else {}))
    _params(fx, c.s)
    b = _build(fx, c, c.own.x, wrap=False)
    lst, nall = fx.pair_get_list()
    _, ng, owner, _ = fx.ghost_get()
    at0 = _atoms(c, _host(b.d_x)[:nall], _host(b.d_q)[:nall], owner)
    fx.close()
    return SimpleNamespace(c=c, at0=at0, lst0=lst)


def new_handle(kind, newton, setup=True, linalg=True, **kw):
    si = setup_inputs(kind, newton)
    c = si.c
    fx = FixConp(c.s, **dict(PPPM if kind == "il_onelayer" else {}, **kw))
    _params(fx, c.s)
    if setup:
        at0 = dataclasses.replace(si.at0, q=si.at0.q.copy())        # (the host-array update writes the electrode charges into its atoms)
        fx.init_lists(si.lst0, si.lst0)
        fx.setup_post_neighbor(at0)
        if linalg:
            fx.setup_pre_force(at0, 0, c.s.potdiff)
    return fx


def _update(fx, b, potdiff):
    """one device-resident update on a fresh copy of the arrays' charges -> (q [nall], eleallq, scalar)"""
    import torch
    d_q = b.q0.clone()
    torch.cuda.synchronize()
    fx.pre_force_device(b.d_x.data_ptr(), d_q.data_ptr(), potdiff)
    torch.cuda.synchronize()
    return SimpleNamespace(q=_host(d_q)[:b.nall], eleallq=fx.vectors()[1].copy(), scalar=fx.compute_scalar())


def device_route(fx, c, x1=None):
    b = _build(fx, c, c.x1 if x1 is None else x1)
    fx.post_neighbor_device(b.d_x.data_ptr(), b.d_q.data_ptr())
    return b


def host_route(fh, c, fd, b):
    """handle fh re-neighboured by the host hook with fd's list and ghosts and the host copies of the arrays b"""
    lst, nall = fd.pair_get_list()
    _, ng, owner, _ = fd.ghost_get()
    assert nall == b.nall and ng == b.nghost
    at1 = _atoms(c, _host(b.d_x)[:nall], _host(b.q0)[:nall], owner)
    fh.init_list(2, lst)
    fh.post_neighbor(at1)
    return at1, lst


def _info(fx):
    i = fx.info()
    return dict(zn_cols=i.zn_cols, zn_grid=i.zn_grid, zn_rows=i.zn_rows, zn_ranges=i.zn_ranges, n_blist_pairs=i.n_blist_pairs,
                n_elyte_charged=i.n_elyte_charged, hc_arithmetic=i.hc_arithmetic)


def _same_tables(tag, a, b):
    for k in a:
        va, vb = a[k], b[k]
        same = np.array_equal(va, vb) if isinstance(va, np.ndarray) else va == vb
        assert same, f"{tag}: {k} differs"


def _same_update(tag, a, b, exact):
    scale = np.abs(a.eleallq).max()
    dq = max(np.abs(a.q - b.q).max(), np.abs(a.eleallq - b.eleallq).max())
    print(f"{tag}: largest charge difference {dq:.3e} (largest charge {scale:.3e}), scalars {a.scalar!r} {b.scalar!r}")
    assert scale > 0 and np.all(np.isfinite(a.q))
    if exact:
        assert a.q.tobytes() == b.q.tobytes() and a.eleallq.tobytes() == b.eleallq.tobytes() and a.scalar == b.scalar, tag
    else:
        assert dq <= TOL_Q * scale and abs(a.scalar - b.scalar) <= TOL_Q * max(abs(a.scalar), scale), tag


def _against_reference(c, t, lst, zn):
    """the tables t against tests/post_neighbor_ref.py at the case's moved, wrapped positions; lst: the list the handle used"""
    e = pnr.expected(c)
    a2e = np.concatenate([c.a2e, c.a2e[c.ghosts.owner]])
    br = pnr.b_rows(lst, a2e, c.n, c.newton, c.ne)
    assert t["nall"] == c.nall and t["ne"] == c.ne and t["nl"] == len(e.elyte) and t["n_ele_atoms"] == len(e.ele_pairs)
    for k in ("ele_pairs", "csr_ptr", "csr_of", "csr_row"):
        assert np.array_equal(t[k], getattr(e, k)), k
    for k in ("b_rowptr", "b_ele", "b_oth"):
        assert np.array_equal(t[k], getattr(br, k)), k
    assert t["n_b_pairs"] == len(br.b_ele) and t["n_b_pairs"] > 0
    if not zn:
        assert t["zn_listed"] == 0 and np.array_equal(t["elyte_idx"], e.elyte)
        return None
    n, lz = pnr.zn_setup(c)
    r = pnr.z_order(c.xw[e.elyte, 2], n, lz)
    assert r.margin >= 1e-9
    assert t["zn_listed"] == 1 and t["c_start"] == r.c_start and t["n_chunks"] == max(32, (len(e.elyte) + 31) // 32 * 32) // 16
    assert np.array_equal(t["elyte_idx"], e.elyte[r.order])
    return n


CASES = [("small", False), ("small", True), ("small127", False), ("small127", True), ("sparse", False), ("medium", False), ("ragged", False),
         ("rough", False), ("il_onelayer", False)]


@pytest.mark.parametrize("kind,newton", CASES)
def test_device_route_equals_the_host_route(kind, newton):
    si = setup_inputs(kind, newton)
    c = si.c
    zn = kind in pnr.MEDIUM
    fd, fh, fh2 = (new_handle(kind, newton) for _ in range(3))
    b = device_route(fd, c)
    assert b.nall == c.nall and np.array_equal(fd.ghost_get()[2], c.ghosts.owner)       # the ghosts are the reference's
    assert np.array_equal(_host(b.d_x)[:c.nall], c.ghosts.x)
    td, idv = fd.step_tables(), _info(fd)
    fd.post_neighbor_device(b.d_x.data_ptr(), b.d_q.data_ptr())                          # the same call again: the same bytes
    td2 = fd.step_tables()
    for k in FixConp.STEP_TABLES:
        assert td[k].tobytes() == td2[k].tobytes(), k
    at1, lst = host_route(fh, c, fd, b)
    host_route(fh2, c, fd, b)
    th, ih = fh.step_tables(), _info(fh)
    _same_tables(f"{kind}: device against host route", td, th)
    _same_tables(f"{kind}: info", idv, ih)
    n = _against_reference(c, td, lst, zn)
    if zn:
        assert idv["zn_cols"] in (32, 48) and ih["zn_cols"] in (32, 48) and idv["zn_grid"] == n
        if kind == "ragged":
            assert td["nl"] == 16379 and td["c_start"] != 0
        if kind == "rough":
            assert fd.info().n_zclasses == 0
    else:
        assert idv["zn_cols"] == 0
    # the control: two host-route handles
    uh, uh2 = _update(fh, b, c.s.potdiff), _update(fh2, b, c.s.potdiff)
    exact = uh.q.tobytes() == uh2.q.tobytes() and uh.eleallq.tobytes() == uh2.eleallq.tobytes() and uh.scalar == uh2.scalar
    if not exact:
        print(f"{kind}: two host-route handles already differ: the bound {TOL_Q} of tests/test_gpu_parity.py takes the place of byte identity")
        _same_update(f"{kind}: control, two host-route handles", uh, uh2, False)
    ud = _update(fd, b, c.s.potdiff)
    _same_update(f"{kind}: device against host route", ud, uh, exact)
    ele = at1.echeck != 0
    assert np.array_equal(ud.q[~ele], _host(b.q0)[:c.nall][~ele])                        # only electrode atoms were written
    if kind == "medium":
        _drift_against_classic(si, fd, b)
    for f in (fd, fh, fh2):
        f.close()


def _drift_against_classic(si, fd, b):
    """five drift steps without a re-neighbour (+-0.25 A in z each, 1.25 A in all: inside the 2.5 A the windows allow) on the handle
    the device entry re-neighboured, against a handle on the full kernels re-neighboured by the host hook: the bound of
    tests/test_gpu_zwindow.py, 1e-9 of the largest charge"""
    import torch
    c = si.c
    rng = np.random.default_rng(8)
    sol = torch.from_numpy(np.nonzero(c.own.echeck == 0)[0]).cuda()
    with capi.test_paths(capi.PATH_SK_CLASSIC):                       # (read at the list build: this handle's list is not z-ordered)
        fc = new_handle("medium", False)
        host_route(fc, c, fd, b)
    assert fc.info().zn_cols == 0
    for step in range(5):
        dz = torch.from_numpy(rng.uniform(-0.25, 0.25, size=len(sol))).cuda()
        b.d_x[sol, 2] += dz
        torch.cuda.synchronize()
        fd.ghost_fill_device(b.d_x.data_ptr(), 0)
        torch.cuda.synchronize()
        uc, ud = _update(fc, b, c.s.potdiff), _update(fd, b, c.s.potdiff)
        assert fd.info().zn_cols in (32, 48) and fc.info().zn_cols == 0
        scale = np.abs(uc.eleallq).max()
        err = np.abs(ud.eleallq - uc.eleallq).max()
        print(f"drift step {step}: z-window against full kernels {err / scale:.3e} of the largest charge")
        assert err < 1e-9 * scale
    fc.close()


def test_two_device_reneighbours_the_second_longer():
    """the second neighbouring has a cutoff 2 A longer for ghosts and list: more ghosts and pairs than the setup or the first had, every
    buffer grows, the tables are the host route's"""
    kind, newton = "small", False
    c1, c2 = pnr.case(kind, newton), pnr.case(kind, newton, 43, 2.0)
    fd, fh = new_handle(kind, newton), new_handle(kind, newton)
    device_route(fd, c1)
    n1 = fd.step_tables()["n_b_pairs"]
    nn1 = fd.pair_get_list()[0].npairs
    b = device_route(fd, c2)
    assert fd.pair_get_list()[0].npairs > nn1
    td = fd.step_tables()
    _, lst = host_route(fh, c2, fd, b)
    _same_tables("second re-neighbour", td, fh.step_tables())
    _against_reference(c2, td, lst, False)
    assert td["n_b_pairs"] != n1
    _same_update("second re-neighbour", _update(fd, b, c2.s.potdiff), _update(fh, b, c2.s.potdiff), True)
    fd.close(); fh.close()


def test_a_list_build_without_the_fix_entry_leaves_the_previous_tables_in_use():
    """the lifetime rule of the header: the fix holds COPIES of the list; conp_pair_build_list_device and conp_ghost_build_device for
    the next neighbouring replace the pair style's list and the ghost map only, and updates with the arrays of the previous
    neighbouring give the same bytes until conp_fix_post_neighbor_device is called"""
    kind, newton = "small", False
    c1, c2 = pnr.case(kind, newton), pnr.case(kind, newton, 43, 2.0)
    fd = new_handle(kind, newton)
    b1 = device_route(fd, c1)
    t1, u1 = fd.step_tables(), _update(fd, b1, c1.s.potdiff)
    b2 = _build(fd, c2, c2.x1)                                        # a new list and new ghosts, no conp_fix_post_neighbor_device
    t1b, u1b = fd.step_tables(), _update(fd, b1, c1.s.potdiff)
    _same_tables("after a list build alone", t1, t1b)
    _same_update("after a list build alone", u1, u1b, True)
    fd.post_neighbor_device(b2.d_x.data_ptr(), b2.d_q.data_ptr())
    assert fd.step_tables()["nall"] == b2.nall
    fd.close()


def test_a_window_overflow_before_the_reneighbour_is_reported_once():
    """an electrolyte atom jumps 60 A in z: the update that follows raises the flag on the device; the re-neighbour completes, returns
    CONP_ERR_NUMERIC once, and leaves a ready handle -- what the header says of conp_fix_post_neighbor"""
    import torch
    kind = "medium"
    c = pnr.case(kind, False)
    fd = new_handle(kind, False)
    b = device_route(fd, c)
    assert fd.info().zn_cols in (32, 48)
    j = int(pnr.elyte_list(c.a2e, c.own.q)[17])
    b.d_x[j, 2] += 60.0
    torch.cuda.synchronize()
    _update(fd, b, c.s.potdiff)                                        # uses the window; no error yet
    x_new = _host(b.d_x)[:c.n].copy()
    b2 = _build(fd, c, x_new)
    with pytest.raises(ConpError) as e:
        fd.post_neighbor_device(b2.d_x.data_ptr(), b2.d_q.data_ptr())
    assert e.value.code == -4 and "z-window" in str(e.value)
    t = fd.step_tables()
    assert fd.info().zn_cols in (32, 48) and t["nall"] == b2.nall
    u = _update(fd, b2, c.s.potdiff)                                   # the handle is ready
    fd.post_neighbor_device(b2.d_x.data_ptr(), b2.d_q.data_ptr())     # ... and the error is not repeated
    _same_tables("after the reported overflow", t, fd.step_tables())
    _same_update("after the reported overflow", u, _update(fd, b2, c.s.potdiff), True)
    fd.close()


def test_refusals_leave_the_handle_as_it_was():
    kind, newton = "small", False
    c = pnr.case(kind, newton)
    si = setup_inputs(kind, newton)
    fd = new_handle(kind, newton)
    b = device_route(fd, c)
    t0, u0 = fd.step_tables(), _update(fd, b, c.s.potdiff)

    def refused(code, what, d_x=None, d_q=None):
        with pytest.raises(ConpError) as e:
            fd.post_neighbor_device(b.d_x.data_ptr() if d_x is None else d_x, b.d_q.data_ptr() if d_q is None else d_q)
        assert e.value.code == code, (what, str(e.value))
        _same_tables(what, t0, fd.step_tables())
        _same_update(what, u0, _update(fd, b, c.s.potdiff), True)

    with pytest.raises(ConpError) as e:                               # (ctypes passes None as NULL)
        fd._check(fd.lib.conp_fix_post_neighbor_device(fd.h, None, capi.C.c_void_p(b.d_q.data_ptr())))
    assert e.value.code == -1
    with pytest.raises(ConpError) as e:
        fd._check(fd.lib.conp_fix_post_neighbor_device(fd.h, capi.C.c_void_p(b.d_x.data_ptr()), None))
    assert e.value.code == -1
    _same_tables("NULL arguments", t0, fd.step_tables())
    # the list and the ghost map for another nlocal
    _build(fd, c, c.x1, nlocal=c.n - 1)
    refused(-2, "nlocal of the list and the ghosts")
    # the list's nall is not nlocal + nghost of the map
    _build(fd, c, c.x1, with_ghosts=False)
    refused(-2, "nall of the list")
    # a list shorter than the fix's cutoff: the pair style's own tables allow it, the fix does not
    _params(fd, c.s, scale=0.5)
    short = SimpleNamespace(**dict(vars(c), cutneigh=0.6 * c.s.cutoff))
    _build(fd, short, c.x1)
    refused(-2, "cutneigh below cut_coul")
    _params(fd, c.s)
    # a refused list build leaves the handle without a list
    with pytest.raises(ConpError):
        fd.pair_build_list_device(b.d_x.data_ptr(), c.n, b.nall, 0.5 * c.s.cutoff)
    refused(-2, "no list")
    # (the list's newton setting cannot differ: conp_pair_build_list_device takes it from the handle)
    b = device_route(fd, c)                                           # everything in order again
    _same_tables("the accepted call", t0, fd.step_tables())
    fd.close()
    # no ghost map / no list at all; before the host setup; before linalg_setup; a decomposed handle
    fx = new_handle(kind, newton)
    at0 = si.at0
    d_x, d_q = _dev(at0.x, np.float64), _dev(at0.q, np.float64)
    for step in ("nothing built", "ghosts only"):
        with pytest.raises(ConpError) as e:
            fx.post_neighbor_device(d_x.data_ptr(), d_q.data_ptr())
        assert e.value.code == -2, step
        fx.ghost_build_device(d_x.data_ptr(), c.n, *c.box)
    fx.close()
    for kw, what in ((dict(setup=False), "before the host setup"), (dict(linalg=False), "before linalg_setup")):
        fx = new_handle(kind, newton, **kw)
        _build(fx, c, c.own.x, wrap=False)
        with pytest.raises(ConpError) as e:
            fx.post_neighbor_device(d_x.data_ptr(), d_q.data_ptr())
        assert e.value.code == -2, what
        fx.close()
    fx = new_handle(kind, newton, setup=False)
    comm = capi.conp_comm(ctx=None, rank=0, nranks=1)                 # (one rank: no callback is ever called)
    fx._check(fx.lib.conp_fix_set_comm(fx.h, capi.C.byref(comm)))
    _build(fx, c, c.own.x, wrap=False)
    with pytest.raises(ConpError) as e:
        fx.post_neighbor_device(d_x.data_ptr(), d_q.data_ptr())
    assert e.value.code == -2 and "decomposed" in str(e.value)
    fx.close()


def test_host_array_entries_refuse_until_a_host_post_neighbor():
    """after the device entry the host copies of the lists are those of the neighbouring before: the host-array update refuses
    (CONP_ERR_STATE, naming the remedy) instead of computing with them; after conp_fix_post_neighbor it works and gives the charges of
    the device-resident update (the same kernels on the same tables: 1e-12 of the largest charge allows for the host hooks' own
    launch grouping and nothing else)"""
    kind, newton = "small", False
    c = pnr.case(kind, newton)
    fd = new_handle(kind, newton)
    b = device_route(fd, c)
    ud = _update(fd, b, c.s.potdiff)
    lst, nall = fd.pair_get_list()
    at1 = _atoms(c, _host(b.d_x)[:nall], _host(b.q0)[:nall], fd.ghost_get()[2])
    for call in (lambda: fd.pre_force(at1, 1, c.s.potdiff), lambda: fd.b_cal(at1), lambda: fd.update_charge(at1),
                 lambda: fd.post_force(at1), lambda: fd.post_force_step(at1, 1), lambda: fd.km_b_cal(at1),
                 lambda: fd.setup_pre_force(at1, 1, c.s.potdiff)):
        with pytest.raises(ConpError) as e:
            call()
        assert e.value.code == -2 and "conp_fix_post_neighbor" in str(e.value)
    f, ev, *_ = fd.pair_compute(at1, eatom=False, vatom=False)        # an entry that uploads its own atoms keeps working
    assert np.all(np.isfinite(f)) and np.abs(f).max() > 0
    _same_update("the device entries after the refusals", ud, _update(fd, b, c.s.potdiff), True)
    fd.init_list(2, lst)
    fd.post_neighbor(at1)
    fd.pre_force(at1, 1, c.s.potdiff)
    ele = at1.echeck != 0
    scale = np.abs(ud.q[ele]).max()
    assert np.abs(at1.q[ele] - ud.q[ele]).max() <= 1e-12 * scale
    fd.post_force(at1)
    fd.close()
