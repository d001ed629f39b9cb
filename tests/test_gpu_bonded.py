"""-m gpu: conp_bonded_compute / conp_bonded_compute_device -- harmonic bonds and angles against the longdouble
reference of tests/bonded_ref.py, entry-wise to 1e-12 of the cancellation-free magnitude.

Every case runs the host entry and the device entry; the device entry runs three times on one stream with one synchronisation, d_f
pre-filled with random values; all outputs are byte-identical between the calls and between the two entries; each output alone, and
all NULL.  Then the state rules and refusals, and a whole device step with the bonded term in it."""
import ctypes as C
import functools

import numpy as np
import pytest

from conp_amd import ConpError, FixConp, capi, neighbor, systems
import bonded_ref as br

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
NAMES = ("f", "ev", "eatom", "vatom")


@functools.lru_cache(maxsize=None)
def handle():
    """one handle for every case: the entries need nothing of the fix but its stream, and no setup call is made on it"""
    return FixConp(systems.small_random(ne_side=4, n_elyte=64))


def atoms_of(c):
    z = np.zeros(c.nall, dtype=np.int32)
    return neighbor.Atoms(nlocal=c.nlocal, nghost=c.nall - c.nlocal, x=c.x, q=np.zeros(c.nall), type=z + 1, tag=z.copy(), echeck=z.copy(),
                          owner=z.copy())


def set_case(fx, c):
    fx.bonded_set_params(c.p.bond_k, c.p.bond_r0, c.p.angle_k, c.p.angle_theta0, newton_bond=c.newton)
    fx.bonded_set_lists(c.nlocal, c.nall, c.bonds, c.angles, c.prd)


def device_call(fx, d_x, nall, pre=None, times=1, f=True, ev=True, eatom=True, vatom=True):
    """`times` calls, each with output tensors of its own (d_f a copy of `pre`, or zeros; the overwritten ones NaN), NO
    synchronisation between them and one afterwards -> a list of (f, eng, W, eatom, vatom) numpy tuples, None where NULL"""
    import torch
    nan = float("nan")
    sets = []
    for _ in range(times):
        d_f = (torch.zeros((nall, 3), dtype=torch.float64, device="cuda") if pre is None else torch.from_numpy(pre.copy()).cuda()) if f else None
        d_ev = torch.full((8,), nan, dtype=torch.float64, device="cuda") if ev else None
        d_e = torch.full((nall,), nan, dtype=torch.float64, device="cuda") if eatom else None
        d_v = torch.full((nall, 6), nan, dtype=torch.float64, device="cuda") if vatom else None
        sets.append((d_f, d_ev, d_e, d_v))
    torch.cuda.synchronize()
    ptr = lambda t: t.data_ptr() if t is not None else 0
    for d_f, d_ev, d_e, d_v in sets:
        fx.bonded_compute_device(d_x.data_ptr(), ptr(d_f), ptr(d_ev), ptr(d_e), ptr(d_v))
    torch.cuda.synchronize()
    outs = []
    for s in sets:
        o = [None if t is None else t.cpu().numpy() for t in s]
        outs.append((o[0], None if o[1] is None else o[1][:2], None if o[1] is None else o[1][2:], o[2], o[3]))
    return outs


def same_bytes(a, b):
    return all((u is None and v is None) or u.tobytes() == v.tobytes() for u, v in zip(a, b))


def run_case(c, fx=None):
    """-> the largest fraction of the bound per output over the entries of this case"""
    import torch
    fx = fx or handle()
    set_case(fx, c)
    R = br.for_case(c)
    at = atoms_of(c)
    worst = {}

    def note(fr):
        for k, v in fr.items():
            worst[k] = max(worst.get(k, 0.0), v)
    host = fx.bonded_compute(at)
    note(br.check(c.tag + ", host entry", host, R))
    d_x = torch.from_numpy(c.x).cuda()
    dev0 = device_call(fx, d_x, c.nall)[0]
    note(br.check(c.tag + ", device entry", dev0, R))
    assert same_bytes(host, dev0), c.tag                                 # the two entries, from f = 0
    pre = np.random.default_rng(2).normal(size=(c.nall, 3))
    three = device_call(fx, d_x, c.nall, pre=pre, times=3)
    assert same_bytes(three[0], three[1]) and same_bytes(three[0], three[2]), c.tag
    host_pre = fx.bonded_compute(at, f=pre.copy())
    assert same_bytes(host_pre, three[0]), c.tag                         # ... and from a pre-filled f
    # the rounding of the one add per atom and of the subtraction below: half an ulp of the sum each
    slack = EPS * (np.abs(pre) + np.abs(R.f.astype(float)))
    br.check(c.tag + ", device entry, pre-filled d_f", (three[0][0] - pre, None, None, None, None), R, slack=slack)
    assert same_bytes(three[0][1:], dev0[1:]), c.tag                     # overwritten outputs do not depend on d_f
    # rows of atoms without a contribution: d_f untouched bit for bit, eatom / vatom exactly 0.0
    idle = np.all(R.A == 0, axis=1) & (R.eatom_abs == 0)
    assert idle.any(), c.tag
    assert three[0][0][idle].tobytes() == pre[idle].tobytes()
    assert not dev0[3][idle].any() and not dev0[4][idle].any() and not np.signbit(dev0[3][idle]).any()
    # each output alone
    for name in NAMES:
        only = device_call(fx, d_x, c.nall, **{m: m == name for m in NAMES})[0]
        assert same_bytes([o for o in only if o is not None], [d for d, o in zip(dev0, only) if o is not None]), (c.tag, name)
    for k, name in enumerate(("forces", "eng", "virial", "eatom", "vatom")):
        got = fx.bonded_compute(at, **{m: m == name for m in ("forces", "eng", "virial", "eatom", "vatom")})
        assert [g is not None for g in got] == [j == k for j in range(5)] and got[k].tobytes() == host[k].tobytes(), (c.tag, name)
    # all NULL: CONP_OK (anything else raises), nothing done
    fx.bonded_compute_device(d_x.data_ptr(), 0, 0, 0, 0)
    fx.bonded_compute(at, forces=False, eng=False, virial=False, eatom=False, vatom=False)
    print(f"{c.tag}: largest fraction of the 1e-12 bound: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    return worst


@pytest.mark.parametrize("form", ["ghost", "image"])
@pytest.mark.parametrize("newton", [True, False])
def test_molecules(newton, form):
    """(what these inputs contain -- molecules through every periodic face and one edge, s = +-1 in x and y, terms with 0, 1 and 2
    owned members of 2 and of 3 -- is asserted from the lists in tests/test_bonded_ref_math.py, without a GPU)"""
    c = br.molecules(newton, form)
    run_case(c)
    if form == "image":                                                  # nothing lands on a ghost row: no fold is needed
        assert c.nall == c.nlocal


def test_ghost_rows_fold_onto_the_closest_image_result():
    """the same molecules in both forms: the ghost-index forces, folded, are the closest-image forces to the bound"""
    import torch
    fx = handle()
    ci, cg = br.molecules(True, "image"), br.molecules(True, "ghost")
    nb, na = len(ci.bonds), len(ci.angles)
    fx.bonded_set_params(cg.p.bond_k, cg.p.bond_r0, cg.p.angle_k, cg.p.angle_theta0, newton_bond=True)
    fx.bonded_set_lists(cg.nlocal, cg.nall, cg.bonds[:nb], cg.angles[:na])           # (without the ghost-only terms)
    f = fx.bonded_compute(atoms_of(cg), eng=False, virial=False, eatom=False, vatom=False)[0]
    assert np.any(f[cg.nlocal:] != 0)
    Ri = br.for_case(ci)
    Rg = br.reference(cg.x, cg.nlocal, cg.bonds[:nb], cg.angles[:na], cg.p, True)
    folded_A = br.fold(Rg.A, cg.owner, cg.nlocal)                        # (equal to the closest-image magnitudes: test_bonded_ref_math)
    assert br.frac("ghost-index forces, folded", br.fold(f, cg.owner, cg.nlocal), Ri.f, br.TOL * folded_A + 1e-17 * folded_A) <= 1.0


def test_hub():
    run_case(br.hub())


@pytest.mark.parametrize("shape", br.EDGE_SHAPES, ids=lambda s: f"{s[0]}b-{s[1]}a-{s[2]}n")
def test_block_edges(shape):
    run_case(br.edges(*shape))


def test_block_edges_newton_off():
    run_case(br.edges(172, 85, 2 * br.BLOCK + 1, newton=False))


def test_degenerate_and_ill_conditioned_terms():
    c = br.degenerate()
    run_case(c)
    host = handle().bonded_compute(atoms_of(c))
    assert np.all(np.isfinite(host[0])) and not host[0][:2].any()        # the bond of length 0: no force
    assert host[3][0] == 0.5 * (c.p.bond_k[0] * c.p.bond_r0[0] ** 2)     # ... and ebond = k r0^2, half of it per member


# ---- state ------------------------------------------------------------------------------------------------------------------------
def _raises(code, fn, *a, **k):
    with pytest.raises(ConpError) as e:
        fn(*a, **k)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_empty_lists_on_a_handle_without_a_setup_call():
    import torch
    fx = FixConp(systems.small_random(ne_side=4, n_elyte=64))
    fx.bonded_set_params()                                               # no types at all
    fx.bonded_set_lists(5, 7)
    x = np.random.default_rng(1).normal(size=(7, 3))
    pre = np.random.default_rng(2).normal(size=(7, 3))
    c = br._case("empty", x, 5, None, None)
    got = device_call(fx, torch.from_numpy(x).cuda(), 7, pre=pre)[0]
    assert got[0].tobytes() == pre.tobytes()
    assert all(not g.any() and not np.signbit(g).any() for g in got[1:])
    host = fx.bonded_compute(atoms_of(c), f=pre.copy())
    assert same_bytes(host, got)
    fx.bonded_set_lists(0, 0)                                            # no atoms either
    d_ev = torch.full((8,), float("nan"), dtype=torch.float64, device="cuda")
    fx.bonded_compute_device(d_ev.data_ptr(), 0, d_ev.data_ptr(), 0, 0)
    torch.cuda.synchronize()
    assert not d_ev.cpu().numpy().any()
    fx.close()


def test_refusals_and_state():
    import torch
    c, h = br.molecules(True, "image"), br.hub()
    fx = FixConp(systems.small_random(ne_side=4, n_elyte=64))
    lib = fx.lib
    at, d_x = atoms_of(c), torch.from_numpy(c.x).cuda()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))

    def lists(**k):
        v = dict(nlocal=c.nlocal, nall=c.nall, nbond=len(c.bonds), bond=ip(c.bonds), nangle=len(c.angles), angle=ip(c.angles),
                 prd=(C.c_double * 3)(*c.prd))
        v.update(k)
        return lib.conp_bonded_set_lists(fx.h, C.byref(capi.conp_bonded_lists(**v)))
    # before set_params: the compute entries and set_lists are out of order
    _raises(-2, fx.bonded_compute, at)
    _raises(-2, fx.bonded_compute_device, d_x.data_ptr(), 0, 0, 0, 0)
    assert lists() == -2
    set_case(fx, c)
    want = fx.bonded_compute(at)
    br.check("before the refusals", want, br.for_case(c))

    def still_fine():
        set_case(fx, c)
        assert same_bytes(fx.bonded_compute(at), want)
    # set_params: NULL struct, NULL table with a positive count, negative count
    assert lib.conp_bonded_set_params(fx.h, None) == -1
    k3 = np.ones(4)
    for bad in (dict(nbondtypes=3, bond_k=dp(k3)), dict(nangletypes=2, angle_theta0=dp(k3)), dict(nbondtypes=-1), dict(nangletypes=-1)):
        assert lib.conp_bonded_set_params(fx.h, C.byref(capi.conp_bonded_params(**bad))) == -1, bad
    assert same_bytes(fx.bonded_compute(at), want)                       # a refused set_params leaves tables and lists as they were
    # set_lists: each refusal leaves the handle without lists, and a valid call gives the unrefused result again
    b_hi, b_neg, b_t0, b_t4 = (c.bonds.copy() for _ in range(4))
    b_hi[5, 1] = c.nall; b_neg[7, 0] = -1; b_t0[3, 2] = 0; b_t4[3, 2] = 4
    a_hi, a_neg, a_t0, a_t3 = (c.angles.copy() for _ in range(4))
    a_hi[2, 2] = c.nall; a_neg[4, 1] = -1; a_t0[1, 3] = 0; a_t3[1, 3] = 3
    nan, inf = float("nan"), float("inf")
    refused = [dict(bond=None), dict(angle=None), dict(nbond=-1), dict(nangle=-1), dict(nlocal=-1), dict(nall=-1),
               dict(nlocal=c.nall + 1), dict(bond=ip(b_hi)), dict(bond=ip(b_neg)), dict(bond=ip(b_t0)), dict(bond=ip(b_t4)),
               dict(angle=ip(a_hi)), dict(angle=ip(a_neg)), dict(angle=ip(a_t0)), dict(angle=ip(a_t3)),
               dict(prd=(C.c_double * 3)(-1.0, 0, 0)), dict(prd=(C.c_double * 3)(0, nan, 0)), dict(prd=(C.c_double * 3)(0, 0, inf))]
    for bad in refused:
        assert lists(**bad) == -1, bad
        _raises(-2, fx.bonded_compute, at)
        _raises(-2, fx.bonded_compute_device, d_x.data_ptr(), 0, 0, 0, 0)
        still_fine()
    assert lib.conp_bonded_set_lists(fx.h, None) == -1
    _raises(-2, fx.bonded_compute, at)
    still_fine()
    # the compute entries: NULL d_x / atoms, another atom count
    _raises(-1, fx.bonded_compute_device, 0, 0, 0, 0, 0)
    assert lib.conp_bonded_compute(fx.h, None, None, None, None, None, None) == -1
    _raises(-1, fx.bonded_compute, atoms_of(h))
    short = atoms_of(c); short.nlocal -= 1
    _raises(-1, fx.bonded_compute, short)
    assert same_bytes(fx.bonded_compute(at), want)
    # set_params after set_lists drops the lists (they were checked against the old tables)
    fx.bonded_set_params(c.p.bond_k, c.p.bond_r0, c.p.angle_k, c.p.angle_theta0)
    _raises(-2, fx.bonded_compute, at)
    still_fine()
    # a second set_lists with other lists replaces the first
    fx.bonded_set_lists(h.nlocal, h.nall, h.bonds, h.angles, h.prd)
    br.check("other lists", fx.bonded_compute(atoms_of(h)), br.for_case(h))
    _raises(-1, fx.bonded_compute, at)
    still_fine()
    fx.close()


# ---- the whole device step ----------------------------------------------------------------------------------------------------------
def test_a_whole_step_with_the_bonded_term():
    """ghost_fill -> pre_force_device -> ewald_forces_device -> pair_compute_device -> bonded_compute_device -> post_force_device ->
    ghost_fold_device on one stream with nothing between, on the box and to the bound of tests/test_gpu_post_force_device.py's step
    test: the folded owned forces are the four host entries' sum, folded in numpy"""
    import torch
    import test_gpu_post_force_device as tpf
    import test_gpu_post_neighbor_device as tp
    import pair_force_ref as pref
    from helpers import rel_err
    from types import SimpleNamespace
    c, fd, fh, b, d_q = tpf._device_and_host_handles(True)
    n, nall = b.n, b.nall
    p = pref.lj_tables(c.s.ntypes, c.s.cutoff)
    fd.pair_set_params(p.cutsq, p.cut_coul, None); fh.pair_set_params(p.cutsq, p.cut_coul, None)
    # the electrolyte atoms three at a time, where they are: owned indices and the box lengths, handed over once; soft springs, so
    # that the term is of the size of the others
    el = np.nonzero(c.own.echeck == 0)[0]
    mol = el[:len(el) // 3 * 3].reshape(-1, 3)
    one = np.ones(len(mol), dtype=int)
    bonds = np.concatenate([np.stack([mol[:, 1], mol[:, 0], one], 1), np.stack([mol[:, 1], mol[:, 2], 2 * one], 1)])
    angles = np.stack([mol[:, 0], mol[:, 1], mol[:, 2], one], 1)
    soft = SimpleNamespace(bond_k=np.array([0.4, 0.7]), bond_r0=np.array([3.0, 4.0]), angle_k=np.array([2.0]), angle_theta0=np.array([1.9]))
    prd = np.where(c.s.periodic, c.s.prd, 0.0)
    for fx in (fd, fh):
        fx.bonded_set_params(soft.bond_k, soft.bond_r0, soft.angle_k, soft.angle_theta0, newton_bond=True)
        fx.bonded_set_lists(n, nall, bonds, angles, prd)
    d_f = torch.zeros((nall, 3), dtype=torch.float64, device="cuda")
    d_out = torch.full((9,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    fd.ghost_fill_device(b.d_x.data_ptr(), d_q.data_ptr())
    fd.pre_force_device(b.d_x.data_ptr(), d_q.data_ptr(), c.s.potdiff)
    fd.ewald_forces_device(b.d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), 0, 0)
    fd.pair_compute_device(b.d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), 0, 0, 0)
    fd.bonded_compute_device(b.d_x.data_ptr(), d_f.data_ptr(), 0, 0, 0)
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
    total += fh.post_force(at1)[0]
    f_bonded = fh.bonded_compute(at1, eng=False, virial=False, eatom=False, vatom=False)[0]
    assert np.abs(f_bonded).max() > 0 and not f_bonded[n:].any()        # owned indices: nothing on a ghost row
    R = br.reference(at1.x, n, bonds, angles, soft, True, prd)
    br.check("the step's bonded term, host entry", (f_bonded, None, None, None, None), R)
    total += f_bonded
    owner = np.asarray(fd.ghost_get()[2], np.int64)
    want = total[:n].copy()
    np.add.at(want, owner, total[n:])
    fr = rel_err(got, want) / tpf.ORACLE
    print(f"a whole step with the bonded term: fraction of the bound {tpf.ORACLE:g}: force {fr:.3g}")
    assert fr < 1.0
    without = (total - f_bonded)[:n].copy()
    np.add.at(without, owner, (total - f_bonded)[n:])
    assert rel_err(got, without) > 1e3 * tpf.ORACLE                      # ... and the sum without the term is far outside the bound
    fd.close(); fh.close()
