"""-m gpu: conp_fix_post_force_device -- the Gaussian correction added straight into device forces, its nine
results left on the device -- against the oracle's post_force, against the host entry conp_fix_post_force on a second handle, and
inside the device-resident call sequences of sections 14 - 19.

Bounds (tests/test_gpu_parity.py::test_post_force_matches_oracle, the project's own): against the oracle forces 1e-9 of the largest
entry, the two energies 1e-9 relative, the virial rtol 1e-9 with atol 1e-9 of its largest entry; against the host entry (the same
arithmetic, another order of the additions) 1e-12 in the same form.  Every comparison prints the fraction of its bound it used."""
import dataclasses
import functools
from types import SimpleNamespace

import numpy as np
import pytest

import oracle_py
from conp_amd import ConpError, FixConp, capi, neighbor, systems
from helpers import OracleRun, rel_err

pytestmark = pytest.mark.gpu

ORACLE, HOST = 1e-9, 1e-12


# ---- inputs ---------------------------------------------------------------------------------------------------------------------------
def pushed_box(lo=0.4):
    """the box of test_post_force_matches_oracle (test_ehgo_pair_mode's with lo = 0.5): six electrolyte atoms 0.4 - 1.1 A from
    electrode atoms -- and three more: one above an electrode atom on the x = 0 face and one below another, both pushed through that
    face (their images across it make the close pairs: a ghost electrolyte neighbour, a ghost electrode neighbour, under either newton
    setting), and one over the middle of a C-C bond"""
    s = systems.small_random(ne_side=4, n_elyte=96, lz=60.0, mode="slab")
    rng = np.random.default_rng(9)
    ele_idx = np.nonzero(s.echeck != 0)[0]; sol_idx = np.nonzero((s.echeck == 0) & (s.q != 0))[0]
    for k in range(6):
        d = rng.normal(size=3); d *= rng.uniform(lo, 1.1) / np.linalg.norm(d)
        s.x[sol_idx[k]] = s.x[ele_idx[3 * k]] + d
    ea, eb, c1, c2 = ele_idx[4], ele_idx[7], ele_idx[1], ele_idx[2]
    assert s.x[ea, 0] == s.boxlo[0] and s.x[eb, 0] == s.boxlo[0]
    assert abs(np.linalg.norm(s.x[c1] - s.x[c2]) - 1.43) < 0.01
    s.x[sol_idx[6]] = s.x[ea] + np.array([-0.5, 0.1, 0.55])
    s.x[sol_idx[7]] = s.x[eb] + np.array([-0.45, -0.1, -0.5])
    s.x[sol_idx[8]] = 0.5 * (s.x[c1] + s.x[c2]) + np.array([0.0, 0.0, 0.3])
    s.x[:, :2] = s.boxlo[:2] + np.mod(s.x[:, :2] - s.boxlo[:2], s.prd[:2])
    return s, SimpleNamespace(bond=(int(c1), int(c2), int(sol_idx[8])))


def listed_pairs(lst):
    own = np.asarray(lst.ilist[:lst.inum], np.int64)
    cnt = lst.numneigh[own].astype(np.int64)
    i = np.repeat(own, cnt)
    start = np.repeat(lst.first[own].astype(np.int64), cnt)
    within = np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt)
    return i, lst.neigh[start + within].astype(np.int64) & neighbor.NEIGHMASK


def contributing(s, at, lst, eta=None):
    """the (i, j) of the listed pairs that contribute, by the rule of the header: exactly one electrode member, inside the pair cutoff,
    eta^2 r^2 < 5.8 -- the products formed one by one in float64, as the kernel forms them"""
    i, j = listed_pairs(lst)
    one = (at.echeck[i] != 0) != (at.echeck[j] != 0)
    i, j = i[one], j[one]
    d = at.x[i] - at.x[j]
    rsq = d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2]
    eta = s.eta if eta is None else eta
    keep = (rsq < s.cutsq_table()[at.type[i], at.type[j]]) & (eta * eta * rsq < 5.8)
    return i[keep], j[keep]


def _dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    torch.cuda.synchronize()
    return t


def call(fx, d_x, d_q, nall, f=True, out=True, pre=None, times=1):
    """`times` calls, each with its own d_out, into ONE d_f, no synchronisation between them and one afterwards -> (d_f as numpy or
    None, [d_out of every call]).  d_out starts as NaN, with a sentinel row behind it that must survive."""
    import torch
    d_f = None if not f else _dev(np.zeros((nall, 3)) if pre is None else pre)
    d_o = [torch.full((10,), float("nan"), dtype=torch.float64, device="cuda") for _ in range(times)] if out else [None] * times
    for t in d_o:
        if t is not None:
            t[9] = -77.0
    torch.cuda.synchronize()
    for k in range(times):
        fx.post_force_device(d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr() if f else 0, d_o[k].data_ptr() if out else 0)
    torch.cuda.synchronize()
    outs = [None if t is None else t.cpu().numpy() for t in d_o]
    for o in outs:
        assert o is None or o[9] == -77.0
    return (None if d_f is None else d_f.cpu().numpy()), [None if o is None else o[:9] for o in outs]


def compare(tag, got_f, got_out, ref_f, ref_ek, ref_ec, ref_vir, tol):
    """the bounds of the module docstring with `tol`; prints and returns the largest fraction of a bound that was used"""
    fr = {}
    if got_f is not None:
        fr["force"] = rel_err(got_f, ref_f) / tol
    if got_out is not None:
        fr["self energy"] = abs(got_out[0] - ref_ek) / (tol * abs(ref_ek))
        fr["eng_coul"] = abs(got_out[1] - ref_ec) / (tol * abs(ref_ec)) if ref_ec != 0.0 else (np.inf if got_out[1] != 0.0 else 0.0)
        vmax = np.abs(ref_vir).max()
        fr["virial"] = float(np.max(np.abs(got_out[2:8] - ref_vir) / (tol * vmax + tol * np.abs(ref_vir)))) if vmax > 0 else \
            (np.inf if np.any(got_out[2:8] != 0.0) else 0.0)
    print(f"{tag}: fractions of the bound {tol:g}: " + ", ".join(f"{k} {v:.3g}" for k, v in fr.items()))
    worst = max(fr.values())
    assert worst < 1.0, (tag, fr)
    return worst


@functools.lru_cache(maxsize=None)
def oracle_case(newton, kind="pushed"):
    """one input through the oracle, through the host entry on a handle of its own, and a handle left ready for the device entry:
    computed once, shared, never written"""
    lib = oracle_py.load()
    if kind == "ehgo":
        from test_gpu_parity import _ehgo_setup
        s, marks = pushed_box(lo=0.5)
        s.newton = newton
        coeffs = [(5, 1.979, 11.0), ("1*2", 1.2, 6.5), (4, 0.9, "auto")]
        at, o, fx = _ehgo_setup(lib, s, 1.0, coeffs)
        ath, oh, fh = _ehgo_setup(lib, s, 1.0, coeffs)
        oh.fx.close()
        _, alist, blist = neighbor.build_lists(s)
        lst = blist
    else:
        s, marks = pushed_box() if kind in ("pushed", "ragged") else (systems.small_random(ne_side=4, n_elyte=96, lz=60.0, mode="slab"), None)
        s.newton = newton
        at, alist, blist = neighbor.build_lists(s)
        lst = blist
        if kind == "ragged":            # the last owner dropped: 159 owners, the last workgroup of the pair kernel has an idle wave
            lst = dataclasses.replace(blist, inum=blist.inum - 1, ilist=blist.ilist[:-1].copy())
            assert lst.inum % 4 != 0
        o = OracleRun(lib, s, at, alist, lst)
        o.setup(); o.pre_force(s.potdiff)
        ath = dataclasses.replace(at, q=at.q.copy())
        fx, fh = FixConp(s), FixConp(s)
        for f, a in ((fx, at), (fh, ath)):
            f.init_lists(alist, lst)
            f.setup_post_neighbor(a)
            f.setup_pre_force(a, 0, s.potdiff)
    f_o, out_o = o.fx.post_force()
    o.fx.close()
    f_h, ek_h, ec_h, vir_h = fh.post_force(ath)
    fh.close()
    ci, cj = contributing(s, at, lst)
    # (the device entry is given the charges the host entry saw: "the same charges" of the header's bit-equality holds by construction)
    return SimpleNamespace(s=s, at=at, lst=lst, fx=fx, marks=marks, f_o=f_o, out_o=out_o, host=(f_h, ek_h, ec_h, vir_h), ci=ci, cj=cj,
                           d_x=_dev(ath.x), d_q=_dev(ath.q))


def check_against_oracle_and_host(tag, c, f_inc, out):
    f_h, ek_h, ec_h, vir_h = c.host
    a = compare(f"{tag}: against the oracle", f_inc, out, c.f_o, c.out_o[0], c.out_o[1], c.out_o[2:8], ORACLE)
    b = compare(f"{tag}: against the host entry", f_inc, out, f_h, ek_h, ec_h, vir_h, HOST)
    if out is not None:
        assert out[0] == ek_h, (out[0], ek_h)                          # bit for bit: the same sum, the same expression
        assert out[8] == float(len(c.ci))
    if f_inc is not None:
        assert np.all(f_inc[c.at.echeck != 0] == 0.0)                  # electrode atoms receive no force from this term
    return a, b


# ---- the oracle's box ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("newton", [False, True])
def test_matches_the_oracle_and_the_host_entry(newton):
    c = oracle_case(newton)
    at, n = c.at, c.at.nlocal
    ele = at.echeck != 0
    # what the input must exercise, from the list and the positions
    assert np.any((c.cj >= n) & ~ele[c.cj]), "no contributing pair with a ghost electrolyte neighbour"
    assert np.any((c.cj >= n) & ele[c.cj]), "no contributing pair with a ghost electrode neighbour"
    assert np.any((c.cj < n) & ele[c.cj])                              # (owned pairs: electrolyte atoms have the lower indices)
    c1, c2, mid = c.marks.bond
    partners = {int(at.owner[j if ele[j] else i]) for i, j in zip(c.ci, c.cj) if at.owner[i if ele[j] else j] == mid}
    assert {c1, c2} <= partners, "the atom over the bond is not inside the gate of both of its atoms"
    nn = c.lst.numneigh[c.lst.ilist[:c.lst.inum]]
    assert np.any((nn > 64) & (nn % 64 != 0)), "no owner with more than 64 neighbours and a ragged last round"
    assert c.lst.inum > 4
    assert np.abs(c.f_o).max() > 1.0
    # one call into pre-filled forces
    pre = np.random.default_rng(3).normal(size=(at.nall, 3))
    f1, (out1,) = call(c.fx, c.d_x, c.d_q, at.nall, pre=pre)
    check_against_oracle_and_host(f"newton {int(newton)}", c, f1 - pre, out1)
    # three calls behind one another, one synchronisation
    f3, outs = call(c.fx, c.d_x, c.d_q, at.nall, pre=pre, times=3)
    compare(f"newton {int(newton)}: three calls against three times the host entry", f3 - pre, None, 3 * c.host[0], 0, 0, 0, HOST)
    compare(f"newton {int(newton)}: three calls against three times the oracle", f3 - pre, None, 3 * c.f_o, 0, 0, 0, ORACLE)
    for o in outs:
        assert o.tobytes() == out1.tobytes()                           # overwritten, never accumulated; a fixed order of additions
    _, (again,) = call(c.fx, c.d_x, c.d_q, at.nall)
    assert again.tobytes() == out1.tobytes()


def test_ehgo_box():
    """the box of test_gpu_parity.py's EHGO case (b): kappa 1, per-type widths, explicit u0"""
    c = oracle_case(False, "ehgo")
    assert len(c.ci) > 0 and np.abs(c.f_o).max() > 0.1
    pre = np.random.default_rng(4).normal(size=(c.at.nall, 3))
    f, (out,) = call(c.fx, c.d_x, c.d_q, c.at.nall, pre=pre)
    check_against_oracle_and_host("ehgo", c, f - pre, out)


def test_no_pair_inside_the_gate():
    c = oracle_case(False, "plain")
    assert len(c.ci) == 0 and not np.any(c.f_o)
    pre = np.random.default_rng(5).normal(size=(c.at.nall, 3))
    f, (out,) = call(c.fx, c.d_x, c.d_q, c.at.nall, pre=pre)
    assert f.tobytes() == pre.tobytes()
    assert np.all(out[1:] == 0.0) and not np.any(np.signbit(out[1:]))
    assert out[0] == c.host[1] and out[0] == pytest.approx(c.out_o[0], rel=ORACLE) and out[0] > 0


def test_an_owner_count_that_is_no_multiple_of_four():
    c = oracle_case(False, "ragged")
    assert c.lst.inum % 4 == 3 and len(c.ci) > 0
    pre = np.random.default_rng(6).normal(size=(c.at.nall, 3))
    f, (out,) = call(c.fx, c.d_x, c.d_q, c.at.nall, pre=pre)
    check_against_oracle_and_host("ragged owner count", c, f - pre, out)


def test_null_outputs():
    c = oracle_case(True)
    nall = c.at.nall
    f_full, (out_full,) = call(c.fx, c.d_x, c.d_q, nall)
    f_only, _ = call(c.fx, c.d_x, c.d_q, nall, out=False)
    _, (out_only,) = call(c.fx, c.d_x, c.d_q, nall, f=False)
    assert out_only.tobytes() == out_full.tobytes()
    compare("d_f alone against the full call", f_only, None, f_full, 0, 0, 0, HOST)
    assert np.array_equal(f_only != 0.0, f_full != 0.0)
    d_f = _dev(np.full((nall, 3), -5.5))
    c.fx.post_force_device(c.d_x.data_ptr(), c.d_q.data_ptr(), 0, 0)        # CONP_OK (anything else raises), nothing done
    import torch
    torch.cuda.synchronize()
    assert np.all(d_f.cpu().numpy() == -5.5)


# ---- behind the device re-neighbour (the two-handle pattern of tests/test_gpu_post_neighbor_device.py) -------------------------------
def _pushed_x1(c):
    """the case's moved positions with four electrolyte atoms pushed onto electrode atoms, and a fifth above an electrode atom of the
    x = 0 face and through that face: its image is the ghost neighbour of that atom under either newton setting (the list build keeps
    an owned-ghost pair where the ghost lies higher in z)"""
    x1 = c.x1.copy()
    rng = np.random.default_rng(12)
    ele = np.nonzero(c.own.echeck != 0)[0]; sol = np.nonzero((c.own.echeck == 0) & (c.own.q != 0))[0]
    for k in range(4):
        d = rng.normal(size=3); d *= rng.uniform(0.4, 1.1) / np.linalg.norm(d)
        x1[sol[20 + k]] = c.own.x[ele[5 * k]] + d
    assert c.own.x[ele[4], 0] == c.box[0][0]
    x1[sol[24]] = c.own.x[ele[4]] + np.array([-0.5, 0.1, 0.55])
    return x1


def _device_and_host_handles(newton):
    """D re-neighboured on the device at the pushed positions, H with the same setup -> (case, D, H, D's device arrays, a fresh copy
    of their charges for the update to write)"""
    import torch
    import post_neighbor_ref as pnr
    import test_gpu_post_neighbor_device as tp
    c = pnr.case("small", newton)
    fd, fh = tp.new_handle("small", newton), tp.new_handle("small", newton)
    b = tp.device_route(fd, c, _pushed_x1(c))
    d_q = b.q0.clone()
    torch.cuda.synchronize()
    return c, fd, fh, b, d_q


def test_after_the_device_reneighbour():
    import torch
    import post_neighbor_ref as pnr
    import test_gpu_post_neighbor_device as tp
    c, fd, fh, b, d_q = _device_and_host_handles(False)
    fd.pre_force_device(b.d_x.data_ptr(), d_q.data_ptr(), c.s.potdiff)
    f_d, (out_d,) = call(fd, b.d_x, d_q, b.nall)
    at1, lst = tp.host_route(fh, c, fd, b)
    at1.q[:] = d_q.cpu().numpy()[:b.nall]
    f_h, ek, ec, vir = fh.post_force(at1)
    assert out_d[8] >= 4 and np.abs(f_h).max() > 0
    ci, _ = contributing(c.s, at1, lst)
    assert out_d[8] == float(len(ci))
    compare("after the device re-neighbour: against the host entry on the same list", f_d, out_d, f_h, ek, ec, vir, HOST)
    assert out_d[0] == ek
    with pytest.raises(ConpError) as e:                                # D's host mirrors are stale: its host entry still refuses
        fd.post_force(at1)
    assert e.value.code == -2 and "conp_fix_post_neighbor" in str(e.value)
    # the lifetime rule: another list for the pair style, at other positions, does not change what the fix walks
    c2 = pnr.case("small", False, 43, 2.0)
    tp._build(fd, c2, c2.x1)
    f_2, (out_2,) = call(fd, b.d_x, d_q, b.nall)
    assert out_2.tobytes() == out_d.tobytes()
    compare("after a list build alone", f_2, None, f_d, 0, 0, 0, HOST)
    fd.close(); fh.close()


def test_a_whole_step_with_nothing_between():
    """pre_force_device -> ewald_forces_device -> pair_compute_device -> post_force_device -> ghost_fold_device on one stream, one
    synchronisation: the folded owned forces are the three host entries' sum, folded in numpy.  Bound: the loosest of the three
    entries' own -- 1e-10 max|f| (tests/test_gpu_ewald_forces.py), 1e-12 A_i (tests/test_gpu_pair_forces.py), 1e-9 max|f|
    (tests/test_gpu_parity.py::test_post_force_matches_oracle) -- 1e-9 of the largest entry"""
    import torch
    import test_gpu_post_neighbor_device as tp
    import pair_force_ref as pref
    c, fd, fh, b, d_q = _device_and_host_handles(True)
    n, nall = b.n, b.nall
    # (coul/long without the LJ part: r^-12 at 0.5 A would bury the term under test far below the bound)
    p = pref.lj_tables(c.s.ntypes, c.s.cutoff)
    fd.pair_set_params(p.cutsq, p.cut_coul, None); fh.pair_set_params(p.cutsq, p.cut_coul, None)
    d_f = torch.zeros((nall, 3), dtype=torch.float64, device="cuda")
    d_out = torch.full((9,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    fd.pre_force_device(b.d_x.data_ptr(), d_q.data_ptr(), c.s.potdiff)
    fd.ewald_forces_device(b.d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), 0, 0)
    fd.pair_compute_device(b.d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), 0, 0, 0)
    fd.post_force_device(b.d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), d_out.data_ptr())
    fd.ghost_fold_device(d_f.data_ptr(), 3)
    torch.cuda.synchronize()
    got = d_f.cpu().numpy()[:n]
    at1, lst = tp.host_route(fh, c, fd, b)
    at1.q[:] = d_q.cpu().numpy()[:nall]
    fh.pair_set_list(lst, nall)
    total = np.zeros((nall, 3))
    total[:n] += fh.ewald_forces(at1, energy=False, virial=False)[0]
    total += fh.pair_compute(at1, eng=False, virial=False, eatom=False, vatom=False)[0]
    f_post = fh.post_force(at1)[0]
    total += f_post
    assert np.abs(f_post).max() > 0 and np.any(f_post[n:] != 0.0) and d_out.cpu().numpy()[8] > 0   # the term acted, on ghost rows too
    want = total[:n].copy()
    np.add.at(want, np.asarray(fd.ghost_get()[2], np.int64), total[n:])
    fr = rel_err(got, want) / ORACLE
    print(f"a whole step: fraction of the bound {ORACLE:g}: force {fr:.3g}")
    assert fr < 1.0
    without = (total - f_post)[:n].copy()
    np.add.at(without, np.asarray(fd.ghost_get()[2], np.int64), (total - f_post)[n:])
    assert rel_err(got, without) > 1e3 * ORACLE                        # ... and the sum without the term is far outside the bound
    fd.close(); fh.close()


def test_refusals():
    import post_neighbor_ref as pnr
    import test_gpu_post_neighbor_device as tp
    c = oracle_case(False)
    nall = c.at.nall
    _, (ref,) = call(c.fx, c.d_x, c.d_q, nall)
    for d_x, d_q in ((0, c.d_q.data_ptr()), (c.d_x.data_ptr(), 0)):
        d_f = _dev(np.full((nall, 3), 2.5))
        with pytest.raises(ConpError) as e:
            c.fx.post_force_device(d_x, d_q, d_f.data_ptr(), 0)
        assert e.value.code == -1
        assert np.all(d_f.cpu().numpy() == 2.5)
        _, (out,) = call(c.fx, c.d_x, c.d_q, nall)
        assert out.tobytes() == ref.tobytes()
    # before setup: the host entry's wording; then the same handle set up gives the result of the handle above
    s, at = c.s, dataclasses.replace(c.at, q=c.at.q.copy())
    _, alist, _ = neighbor.build_lists(s)
    fx = FixConp(s)
    fx.init_lists(alist, c.lst)
    d_o = _dev(np.zeros(9))
    for stage in ("created", "post_neighbor"):
        with pytest.raises(ConpError) as e:
            fx.post_force_device(c.d_x.data_ptr(), c.d_q.data_ptr(), 0, d_o.data_ptr())
        assert e.value.code == -2 and "post_force before setup" in str(e.value), stage
        if stage == "created":
            fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)
    f, (out,) = call(fx, c.d_x, c.d_q, nall)
    f_h, ek_h, ec_h, vir_h = c.host
    compare("after the refusals before setup", f, out, f_h, ek_h, ec_h, vir_h, HOST)
    fx.close()
    # a decomposed handle: update_direct's wording
    fx = tp.new_handle("small", False, setup=False)
    comm = capi.conp_comm(ctx=None, rank=0, nranks=1)                 # (one rank: no callback is ever called)
    fx._check(fx.lib.conp_fix_set_comm(fx.h, capi.C.byref(comm)))
    with pytest.raises(ConpError) as e:
        fx.post_force_device(c.d_x.data_ptr(), c.d_q.data_ptr(), 0, d_o.data_ptr())
    assert e.value.code == -2 and "spatially decomposed" in str(e.value)
    assert not np.any(d_o.cpu().numpy())
    fx.close()
    _, (out,) = call(c.fx, c.d_x, c.d_q, nall)
    assert out.tobytes() == ref.tobytes()
