"""-m gpu: conp_zmirror_set_params / conp_zmirror_post_integrate_device / conp_zmirror_get_map -- the reference's `fix zmirror` on the
device against tests/exclude_ref.py::mirror_map / mirror_apply (checked without a GPU by
tests/test_exclude_ref_math.py).

(1) the map equals mirror_map for 1, 63, 64, 65 and 4097 pairs, groups interleaved in index order and tags shuffled;  (2) x after the
call is bit-equal to mirror_apply; rows outside the receiving group and the rows behind nlocal keep their bytes;  (3) a step with
ntimestep % nevery != 0 changes nothing;  (4) every refusal is followed by a valid call;  (5) the call works after
conp_atoms_wrap_device;  (6) the reference's zmirror deck, conp and conq: steps without and with a device re-neighbouring."""
from types import SimpleNamespace

import numpy as np
import pytest

import exclude_ref as xref
from conp_amd import ConpError, FixConp, capi
from test_gpu_pair_forces import system

pytestmark = pytest.mark.gpu

SEND, RECV = 2, 4
PAIRS = (1, 63, 64, 65, 4097)


def _dev(a, dtype):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()
    torch.cuda.synchronize()
    return t


def _host(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _coords(n_rows, seed):
    """coordinates with every bit pattern class a subtraction can meet: ordinary values, exact zeros, a negative zero, a denormal"""
    x = np.random.default_rng(seed).normal(size=(n_rows, 3)) * 23.0
    x[0, 2] = 0.0
    if n_rows > 3:
        x[1, 2], x[2, 2] = -0.0, 5e-324
    return x


@pytest.mark.parametrize("layout", ["interleaved", "shuffled"])
@pytest.mark.parametrize("n", PAIRS)
def test_ladder_map_and_copy(n, layout):
    """the body the guard test repeats: map, copy, untouched rows, a skipped step"""
    tag, mask = xref.mirror_groups(n, seed=n, layout=layout)
    nlocal, extra = 2 * n, 5                                                    # `extra` rows behind nlocal (ghosts)
    boxlo_z, zprd = -31.25, 71.5
    src, dst = xref.mirror_map(tag, mask, SEND, RECV)
    fx = FixConp(system("small", False))
    fx.zmirror_set_params(tag, mask, SEND, RECV, 3, boxlo_z, zprd)
    gs, gd = fx.zmirror_get_map()
    assert np.array_equal(gs, src) and np.array_equal(gd, dst) and len(gs) == n
    x = _coords(nlocal + extra, seed=100 + n)
    d_x = _dev(x, np.float64)
    fx.zmirror_post_integrate_device(d_x.data_ptr(), 7)                          # 7 % 3 != 0: nothing is launched
    assert _host(d_x).tobytes() == x.tobytes()
    fx.zmirror_post_integrate_device(d_x.data_ptr(), 9)
    got = _host(d_x)
    want = xref.mirror_apply(x, src, dst, 2 * boxlo_z + zprd)
    assert got.tobytes() == want.tobytes()                                       # bit-equal, -0.0 and denormals included
    rest = np.setdiff1d(np.arange(nlocal + extra), dst)
    assert got[rest].tobytes() == x[rest].tobytes() and np.any(got[dst] != x[dst])
    fx.zmirror_post_integrate_device(d_x.data_ptr(), 0)                          # again: the identity (x of the sources has not changed)
    assert _host(d_x).tobytes() == want.tobytes()
    fx.close()


def test_refusals_each_followed_by_a_valid_call():
    n = 8
    tag, mask = xref.mirror_groups(n, seed=4)
    src, dst = xref.mirror_map(tag, mask, SEND, RECV)
    x = _coords(2 * n, 1)
    fx = FixConp(system("small", False))
    d_x = _dev(x, np.float64)
    for call in (lambda: fx.zmirror_post_integrate_device(d_x.data_ptr(), 0), fx.zmirror_get_map):          # before set_params
        with pytest.raises(ConpError) as e:
            call()
        assert e.value.code == -2

    def valid():
        fx.zmirror_set_params(tag, mask, SEND, RECV, 1, -2.0, 9.0)
        d = _dev(x, np.float64)
        fx.zmirror_post_integrate_device(d.data_ptr(), 5)
        assert _host(d).tobytes() == xref.mirror_apply(x, src, dst, 5.0).tobytes()
    valid()
    ok = dict(tag=tag, mask=mask, groupbit=SEND, jgroupbit=RECV, nevery=1, boxlo_z=-2.0, zprd=9.0)
    t2 = tag.copy(); t2[0] = t2[1]
    m_short = mask.copy(); m_short[tag == 2 * n] = 1
    t_gone = tag.copy(); t_gone[tag == 12] = 100
    m_gone = mask.copy(); m_gone[tag == 12] = 1
    tag3 = np.arange(1, 13).astype(np.int32)
    mask3 = np.where(tag3 <= 4, 1 | 2, np.where(tag3 <= 8, 1 | 2 | 4, 1 | 4)).astype(np.int32)
    bad = [dict(groupbit=16), dict(jgroupbit=16), dict(mask=m_short), dict(tag=t_gone, mask=m_gone), dict(mask=m_gone),
           dict(tag=tag3, mask=mask3), dict(nevery=0), dict(nevery=-1), dict(zprd=float("inf")), dict(zprd=float("nan")),
           dict(boxlo_z=float("nan")), dict(tag=t2)]
    for kw in bad:
        a = dict(ok); a.update(kw)
        if not set(kw) & {"nevery", "zprd", "boxlo_z"}:                          # (mirror_map refuses what concerns the map)
            with pytest.raises(ValueError):
                xref.mirror_map(a["tag"], a["mask"], a["groupbit"], a["jgroupbit"])
        with pytest.raises(ConpError) as e:
            fx.zmirror_set_params(**a)
        assert e.value.code == -1, kw
        with pytest.raises(ConpError) as e:                                      # a refused call leaves the handle without a mirror
            fx.zmirror_post_integrate_device(d_x.data_ptr(), 0)
        assert e.value.code == -2, kw
        valid()
    one = (capi.C.c_int * 1)(1)
    ip = capi.C.cast(one, capi.C.POINTER(capi.C.c_int))
    for p in (capi.conp_zmirror_params(nlocal=1, tag=ip, nevery=1, groupbit=1, jgroupbit=1),
              capi.conp_zmirror_params(nlocal=1, mask=ip, nevery=1, groupbit=1, jgroupbit=1),
              capi.conp_zmirror_params(nlocal=-1, tag=ip, mask=ip, nevery=1, groupbit=1, jgroupbit=1)):
        assert fx.lib.conp_zmirror_set_params(fx.h, capi.C.byref(p)) == -1
        valid()
    assert fx.lib.conp_zmirror_set_params(fx.h, None) == -1
    valid()
    with pytest.raises(ConpError) as e:                                          # NULL d_x: refused, the mirror stays
        fx.zmirror_post_integrate_device(0, 0)
    assert e.value.code == -1
    d = _dev(x, np.float64)
    fx.zmirror_post_integrate_device(d.data_ptr(), 0)
    assert _host(d).tobytes() == xref.mirror_apply(x, src, dst, 5.0).tobytes()
    fx.close()


def test_after_the_wrap_entry():
    """conp_atoms_wrap_device remaps in place: owned indices are stable, the map of set_params stays valid"""
    from ghost_ref import wrap
    n = 65
    tag, mask = xref.mirror_groups(n, seed=9)
    src, dst = xref.mirror_map(tag, mask, SEND, RECV)
    boxlo, boxhi, periodic = np.array([-10.0, -12.0, -20.0]), np.array([10.0, 12.0, 20.0]), (True, True, True)
    x = np.random.default_rng(5).uniform(-1.3, 1.3, size=(2 * n, 3)) * (boxhi - boxlo) * 0.5          # some atoms outside the box
    assert np.any(np.abs(x) > 0.5 * (boxhi - boxlo))
    fx = FixConp(system("small", False))
    fx.zmirror_set_params(tag, mask, SEND, RECV, 1, boxlo[2], boxhi[2] - boxlo[2])
    d_x = _dev(x, np.float64)
    fx.atoms_wrap_device(d_x.data_ptr(), 2 * n, boxlo, boxhi, periodic)
    fx.zmirror_post_integrate_device(d_x.data_ptr(), 0)
    xw, _ = wrap(x, boxlo, boxhi, periodic)
    want = xref.mirror_apply(xw, src, dst, 2 * boxlo[2] + (boxhi[2] - boxlo[2]))
    assert _host(d_x).tobytes() == want.tobytes()
    fx.close()


@pytest.mark.parametrize("style,arg", [("conp", 2.0), ("conq", 0.7)])
def test_the_zmirror_deck(style, arg):
    """tests/zmirror/input trial 2 (conp) and 3 (conq) on systems.deck("il_onelayer", "zmirror") with the deck's groups: `fix 2 solneg
    zmirror 1 solpos` and `neigh_modify exclude group solpos solpos`.  (a) solneg moves by less than skin / 2 -> mirror -> ghost fill ->
    update;  (b) solneg moves far enough to set the moved flag -> mirror -> the device re-neighbouring sequence with the excluded
    build -> update.  After each update the mirror relation of x is bit-exact, and the charge of every electrode atom and that of its
    mirror partner (tag + natoms / 2) differ by no more than 4 x the defect the same handle shows at step 0, where the mirror is the
    system builder's (the summation order differs between the halves and nothing else does), and never less than 1e-12 of the
    largest charge.  After (b) the charges equal those of a fresh host-route handle set up from the downloaded coordinates with the
    filter_list-ed host list, to 1e-8 of the largest charge (tests/test_gpu_post_neighbor_device.py::TOL_Q: that handle's rows are in
    another order, so byte identity is not on offer).
    Step-0 defects measured on an MI355X: see DESIGN.md section 25."""
    import torch
    import test_gpu_pair_exclude as tx
    import test_gpu_post_neighbor_device as tpn
    import neigh_ref as nref
    c = tx.zmirror_box()
    n, own = c.n, c.own
    boxlo, boxhi, periodic, cut = c.box
    fx = tx.zmirror_handle(c, style, arg)
    fx.zmirror_set_params(own.tag, own.mask, tx.SOLNEG, tx.SOLPOS, 1, boxlo[2], boxhi[2] - boxlo[2])
    src, dst = fx.zmirror_get_map()
    ws, wd = xref.mirror_map(own.tag, own.mask, tx.SOLNEG, tx.SOLPOS)
    assert np.array_equal(src, ws) and np.array_equal(dst, wd) and np.array_equal(own.tag[dst], own.tag[src] + n // 2)
    zoffset = 2 * boxlo[2] + (boxhi[2] - boxlo[2])
    ele = np.nonzero(own.echeck != 0)[0]
    lower = ele[own.tag[ele] <= n // 2]
    at_tag = np.full(n + 1, -1, np.int64)
    at_tag[own.tag] = np.arange(n)
    partner = at_tag[own.tag[lower] + n // 2]
    assert np.all(partner >= 0) and np.array_equal(own.echeck[partner], own.echeck[lower])

    def defect(u):
        return float(np.abs(u.q[lower] - u.q[partner]).max()), float(np.abs(u.q[ele]).max())

    def mirrored(d_x):
        x = _host(d_x)[:n]
        assert x[dst].tobytes() == np.stack([x[src, 0], x[src, 1], zoffset - x[src, 2]], axis=1).tobytes()
        return x
    # step 0: the device re-neighbouring at x0, the builder's mirror
    b = tx.zmirror_reneighbor(fx, c, _dev(own.x, np.float64), wrap=False)
    d0, scale = defect(tpn._update(fx, b, arg))
    bound = max(4.0 * d0, 1e-12 * scale)
    print(f"{style}: step-0 mirror defect of the electrode charges {d0:.3e} (largest charge {scale:.3e}): bound {bound:.3e}")
    flag = torch.full((1,), 7, dtype=torch.int32, device="cuda")
    rng = np.random.default_rng(17)
    sneg = torch.from_numpy(src.astype(np.int64)).cuda()

    def move(longest):
        step = rng.normal(size=(len(src), 3))
        step *= (longest * rng.uniform(0.2, 1.0, size=len(src)) / np.linalg.norm(step, axis=1))[:, None]
        b.d_x[sneg] += torch.from_numpy(step).cuda()
        torch.cuda.synchronize()
        fx.zmirror_post_integrate_device(b.d_x.data_ptr(), 1)
        fx.pair_list_moved_device(b.d_x.data_ptr(), 0.5 * c.s.skin, flag.data_ptr())
        torch.cuda.synchronize()
        return int(flag.cpu()[0])
    # (a) below skin / 2: no re-neighbouring
    assert move(0.45 * c.s.skin) == 0
    fx.ghost_fill_device(b.d_x.data_ptr(), 0)
    xa = mirrored(b.d_x)
    assert np.any(xa != own.x)
    da, _ = defect(tpn._update(fx, b, arg))
    print(f"{style}: (a) mirror defect of the electrode charges {da:.3e}")
    assert da <= bound
    # (b) past skin / 2: mirror, then the device re-neighbouring sequence with the excluded build
    assert move(0.9 * c.s.skin) == 1
    d_own = b.d_x[:n].clone()
    b = tx.zmirror_reneighbor(fx, c, d_own)
    xb = mirrored(b.d_x)
    ub = tpn._update(fx, b, arg)
    db, _ = defect(ub)
    print(f"{style}: (b) mirror defect of the electrode charges {db:.3e}")
    assert db <= bound
    # a fresh host-route handle at the downloaded coordinates with the filtered host list
    owner = fx.ghost_get()[2]
    full = np.concatenate([np.arange(n), owner]).astype(np.int64)
    at1 = tpn._atoms(c, _host(b.d_x)[:b.nall], _host(b.q0)[:b.nall], owner)
    inp = SimpleNamespace(at=at1, cutneigh=c.cutneigh, newton=False, prd_half=c.prd_half)
    host_list = xref.filter_list(nref.reference(inp)[0], c.rule, own.type[full], own.mask[full], own.molecule[full])
    got, _ = fx.pair_get_list()
    assert np.array_equal(nref.sort_rows(n, got.numneigh, got.neigh), host_list.neigh)
    fh = FixConp(c.s, style=style)
    fh.init_lists(host_list, host_list)
    fh.setup_post_neighbor(at1)
    fh.setup_pre_force(at1, 0, arg)
    err = float(np.abs(at1.q[ele] - ub.q[ele]).max())
    print(f"{style}: device route against a fresh host-route handle {err:.3e} (largest charge {scale:.3e})")
    assert err <= tpn.TOL_Q * scale
    fh.close(); fx.close()
