"""-m gpu: conp_dihedral_compute / conp_dihedral_compute_device -- opls and harmonic dihedrals, harmonic and cvff impropers (DESIGN.md
section 28) against the longdouble reference of tests/dihedral_ref.py, entry-wise to 1e-12 of the cancellation-free magnitude.

Every case runs the host entry and the device entry; the device entry runs three times on one stream with one synchronisation, d_f
pre-filled with random values; all outputs are byte-identical between the calls and between the two entries; each output alone, and
all NULL.  Then the device entry's energy differences against its own force, the state rules and refusals, and a whole device step
with the term in it."""
import ctypes as C
import functools

import numpy as np
import pytest

from conp_amd import ConpError, FixConp, capi, neighbor, systems
import dihedral_ref as dr

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


def set_params(fx, p, newton=True):
    fx.dihedral_set_params(p.dstyle, p.dcoef, p.istyle, p.icoef, newton_bond=newton)


def set_case(fx, c):
    set_params(fx, c.p, c.newton)
    fx.dihedral_set_lists(c.nlocal, c.nall, c.dihedrals, c.impropers, c.prd)


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
        fx.dihedral_compute_device(d_x.data_ptr(), ptr(d_f), ptr(d_ev), ptr(d_e), ptr(d_v))
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
    R = dr.for_case(c)
    at = atoms_of(c)
    worst = {}

    def note(fr):
        for k, v in fr.items():
            worst[k] = max(worst.get(k, 0.0), v)
    host = fx.dihedral_compute(at)
    note(dr.check(c.tag + ", host entry", host, R))
    d_x = torch.from_numpy(c.x).cuda()
    dev0 = device_call(fx, d_x, c.nall)[0]
    note(dr.check(c.tag + ", device entry", dev0, R))
    assert same_bytes(host, dev0), c.tag                                 # the two entries, from f = 0
    pre = np.random.default_rng(2).normal(size=(c.nall, 3))
    three = device_call(fx, d_x, c.nall, pre=pre, times=3)
    assert same_bytes(three[0], three[1]) and same_bytes(three[0], three[2]), c.tag
    host_pre = fx.dihedral_compute(at, f=pre.copy())
    assert same_bytes(host_pre, three[0]), c.tag                         # ... and from a pre-filled f
    # the rounding of the one add per atom and of the subtraction below: half an ulp of the sum each
    slack = EPS * (np.abs(pre) + np.abs(R.f.astype(float)))
    dr.check(c.tag + ", device entry, pre-filled d_f", (three[0][0] - pre, None, None, None, None), R, slack=slack)
    assert same_bytes(three[0][1:], dev0[1:]), c.tag                     # overwritten outputs do not depend on d_f
    # rows of atoms in no term (or, with newton off, of ghosts): d_f untouched bit for bit, eatom / vatom exactly 0.0
    members = np.concatenate([c.dihedrals, c.impropers])[:, :4].reshape(-1)
    idle = np.bincount(members, minlength=c.nall) == 0
    if not c.newton:
        idle[c.nlocal:] = True
    assert idle.any(), c.tag
    assert three[0][0][idle].tobytes() == pre[idle].tobytes()
    assert not dev0[3][idle].any() and not dev0[4][idle].any() and not np.signbit(dev0[3][idle]).any()
    # each output alone
    for name in NAMES:
        only = device_call(fx, d_x, c.nall, **{m: m == name for m in NAMES})[0]
        assert same_bytes([o for o in only if o is not None], [d for d, o in zip(dev0, only) if o is not None]), (c.tag, name)
    for k, name in enumerate(("forces", "eng", "virial", "eatom", "vatom")):
        got = fx.dihedral_compute(at, **{m: m == name for m in ("forces", "eng", "virial", "eatom", "vatom")})
        assert [g is not None for g in got] == [j == k for j in range(5)] and got[k].tobytes() == host[k].tobytes(), (c.tag, name)
    # all NULL: CONP_OK (anything else raises), nothing done
    fx.dihedral_compute_device(d_x.data_ptr(), 0, 0, 0, 0)
    fx.dihedral_compute(at, forces=False, eng=False, virial=False, eatom=False, vatom=False)
    print(f"{c.tag}: largest fraction of the 1e-12 bound: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))
    return worst


@pytest.mark.parametrize("form", ["ghost", "image"])
@pytest.mark.parametrize("newton", [True, False])
@pytest.mark.parametrize("pair", ["opls", "cos"])
def test_molecules(pair, newton, form):
    """(what these inputs contain -- chains through every periodic face and one edge, s = +-1 in x and y, terms with 0 to 4 owned
    members, chi0 = 0 and not 0, n = 0 and n = 3 -- is asserted from the lists in tests/test_dihedral_ref_math.py, without a GPU)"""
    c = dr.molecules(pair, newton, form)
    run_case(c)
    if form == "image":                                                  # nothing lands on a ghost row: no fold is needed
        assert c.nall == c.nlocal


@pytest.mark.parametrize("pair", ["opls", "cos"])
def test_ghost_rows_fold_onto_the_closest_image_result(pair):
    """the same molecules in both forms: the ghost-index forces, folded, are the closest-image forces to the bound"""
    fx = handle()
    ci, cg = dr.molecules(pair, True, "image"), dr.molecules(pair, True, "ghost")
    nd, ni = len(ci.dihedrals), len(ci.impropers)
    set_params(fx, cg.p)
    fx.dihedral_set_lists(cg.nlocal, cg.nall, cg.dihedrals[:nd], cg.impropers[:ni])         # (without the ghost-only terms)
    f = fx.dihedral_compute(atoms_of(cg), eng=False, virial=False, eatom=False, vatom=False)[0]
    assert np.any(f[cg.nlocal:] != 0)
    Ri = dr.for_case(ci)
    Rg = dr.reference(cg.x, cg.nlocal, cg.dihedrals[:nd], cg.impropers[:ni], cg.p, True)
    folded_A = dr.fold(Rg.A, cg.owner, cg.nlocal)                        # (equal to the closest-image magnitudes: test_dihedral_ref_math)
    assert dr.frac("ghost-index forces, folded", dr.fold(f, cg.owner, cg.nlocal), Ri.f, dr.TOL * folded_A + 1e-17 * folded_A) <= 1.0


def test_hub():
    run_case(dr.hub())


@pytest.mark.parametrize("shape", dr.EDGE_SHAPES, ids=lambda s: f"{s[0]}d-{s[1]}i-{s[2]}n-{s[3]}")
def test_block_edges(shape):
    run_case(dr.edge_case(shape))


def test_block_edges_newton_off():
    run_case(dr.edge_case((129, 128, None, "cos"), newton=False))


@pytest.mark.parametrize("pair", ["opls", "cos"])
def test_exact_planar_and_collinear_terms(pair):
    c = dr.exact(pair)
    run_case(c)
    fx = handle()
    at = atoms_of(c)
    host = fx.dihedral_compute(at)
    assert np.all(np.isfinite(host[0]))
    assert not host[0][6:15].any() and not host[3][6:15].any() and not host[4][6:15].any()         # collinear, coinciding: nothing at all
    # the cis and the trans term alone: phi = 0 and phi = pi exactly, so the energies are the closed forms in float64
    if pair == "opls":
        K = c.p.dcoef
        for term, want in ((c.dihedrals[0], K[0, 0] + K[0, 2]), (c.dihedrals[1], 0.0)):
            fx.dihedral_set_lists(c.nlocal, c.nall, [term], None)
            e = fx.dihedral_compute(at, forces=False, virial=False, eatom=False, vatom=False)[1]
            assert abs(e[0] - want) <= 4 * EPS * np.abs(K[term[4] - 1]).sum() and e[1] == 0.0
    else:
        (K, d, n), term = c.p.dcoef[0], c.dihedrals[0]
        fx.dihedral_set_lists(c.nlocal, c.nall, [term], None)
        got = fx.dihedral_compute(at, virial=False, eatom=False, vatom=False)
        assert got[1][0] == K * (1.0 + d) and not got[0].any()           # phi = 0: cos(n phi) = 1, sin(n phi) = 0, no force


def test_the_device_energy_differences_are_the_device_force():
    """the device entry alone: d_ev[0] at x +- h e for a dozen coordinates against the entry's own force, h = 1e-4 A, to 1e-5 of the
    largest force component (tests/test_dihedral_ref_math.py: the reference's own quotient at this h is within a tenth of that)"""
    import torch
    fx = handle()
    c = dr.difference_case()
    set_case(fx, c)
    d_x = torch.from_numpy(c.x).cuda()
    f = device_call(fx, d_x, c.nall, ev=False, eatom=False, vatom=False)[0][0]
    used = np.unique(c.dihedrals[:, :4].reshape(-1))
    rng = np.random.default_rng(4)
    coords = [(int(i), int(d)) for i, d in zip(rng.choice(used, 12, replace=False), rng.integers(0, 3, 12))]
    scale = np.abs(f).max()
    worst = 0.0
    for i, d in coords:
        e = []
        for sign in (1.0, -1.0):
            y = c.x.copy(); y[i, d] += sign * dr.DIFF_H
            d_y = torch.from_numpy(y).cuda()
            e.append(device_call(fx, d_y, c.nall, f=False, eatom=False, vatom=False)[0][1][0])
        g = -(e[0] - e[1]) / (2 * dr.DIFF_H)
        worst = max(worst, abs(g - f[i, d]) / (dr.DIFF_BOUND * scale))
    print(f"device energy differences against the device force: {worst:.3g} of the bound {dr.DIFF_BOUND:g} of {scale:.3g}")
    assert scale > 0 and worst <= 1.0


# ---- state ------------------------------------------------------------------------------------------------------------------------
def _raises(code, fn, *a, **k):
    with pytest.raises(ConpError) as e:
        fn(*a, **k)
    assert e.value.code == code, (e.value.code, str(e.value))


def test_empty_lists_on_a_handle_without_a_setup_call():
    import torch
    fx = FixConp(systems.small_random(ne_side=4, n_elyte=64))
    fx.dihedral_set_params()                                             # no style at all
    fx.dihedral_set_lists(5, 7)
    x = np.random.default_rng(1).normal(size=(7, 3))
    pre = np.random.default_rng(2).normal(size=(7, 3))
    c = dr._case("empty", x, 5, None, None)
    got = device_call(fx, torch.from_numpy(x).cuda(), 7, pre=pre)[0]
    assert got[0].tobytes() == pre.tobytes()
    assert all(not g.any() and not np.signbit(g).any() for g in got[1:])
    host = fx.dihedral_compute(atoms_of(c), f=pre.copy())
    assert same_bytes(host, got)
    fx.dihedral_set_lists(0, 0)                                          # no atoms either
    d_ev = torch.full((8,), float("nan"), dtype=torch.float64, device="cuda")
    fx.dihedral_compute_device(d_ev.data_ptr(), 0, d_ev.data_ptr(), 0, 0)
    torch.cuda.synchronize()
    assert not d_ev.cpu().numpy().any()
    fx.close()


def test_refusals_and_state():
    import torch
    c, h = dr.molecules("opls", True, "image"), dr.hub()
    fx = FixConp(systems.small_random(ne_side=4, n_elyte=64))
    lib = fx.lib
    at, d_x = atoms_of(c), torch.from_numpy(c.x).cuda()
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))
    ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int))
    dt, it = (np.ascontiguousarray(t) for t in dr.table(c.p))
    ct, vt = (np.ascontiguousarray(t) for t in dr.table(dr.PARAMS_COS))

    def lists(**k):
        v = dict(nlocal=c.nlocal, nall=c.nall, ndihedral=len(c.dihedrals), dihedral=ip(c.dihedrals), nimproper=len(c.impropers),
                 improper=ip(c.impropers), prd=(C.c_double * 3)(*c.prd))
        v.update(k)
        return lib.conp_dihedral_set_lists(fx.h, C.byref(capi.conp_dihedral_lists(**v)))

    def params(**k):
        v = dict(dihedral_style=1, ndihedraltypes=len(dt) - 1, dihedral_coef=dp(dt), improper_style=1, nimpropertypes=len(it) - 1,
                 improper_coef=dp(it), newton_bond=1)
        v.update(k)
        return lib.conp_dihedral_set_params(fx.h, C.byref(capi.conp_dihedral_params(**v)))
    # before set_params: the compute entries and set_lists are out of order
    _raises(-2, fx.dihedral_compute, at)
    _raises(-2, fx.dihedral_compute_device, d_x.data_ptr(), 0, 0, 0, 0)
    assert lists() == -2
    assert params() == 0
    _raises(-2, fx.dihedral_compute, at)                                 # ... and with tables but no lists
    set_case(fx, c)
    want = fx.dihedral_compute(at)
    dr.check("before the refusals", want, dr.for_case(c))

    def still_fine():
        set_case(fx, c)
        assert same_bytes(fx.dihedral_compute(at), want)
    # set_params: NULL struct, NULL table with a positive count, negative count, unknown style, types for a style that is 0, a
    # coefficient that is not finite; for the cosine styles d other than +-1, n not an integer, n outside its range
    assert lib.conp_dihedral_set_params(fx.h, None) == -1
    nan_t = dt.copy(); nan_t[2, 1] = float("nan")
    inf_t = it.copy(); inf_t[1, 0] = float("inf")

    def cos_rows(t, col, val, row=1):
        t = t.copy(); t[row, col] = val
        return t
    bad_cos = [cos_rows(ct, 1, 0.0), cos_rows(ct, 1, 2.0), cos_rows(ct, 1, -0.5), cos_rows(ct, 2, 1.5), cos_rows(ct, 2, -1.0),
               cos_rows(ct, 2, 13.0)]
    bad_cvff = [cos_rows(vt, 1, 0.0), cos_rows(vt, 2, 0.5), cos_rows(vt, 2, -1.0), cos_rows(vt, 2, 7.0)]
    refused = [dict(dihedral_coef=None), dict(improper_coef=None), dict(ndihedraltypes=-1), dict(nimpropertypes=-1),
               dict(dihedral_style=3), dict(dihedral_style=-1), dict(improper_style=3), dict(improper_style=-1),
               dict(dihedral_style=0), dict(improper_style=0), dict(dihedral_coef=dp(nan_t)), dict(improper_coef=dp(inf_t))]
    refused += [dict(dihedral_style=2, dihedral_coef=dp(t)) for t in bad_cos]
    refused += [dict(improper_style=2, improper_coef=dp(t)) for t in bad_cvff]
    for bad in refused:
        assert params(**bad) == -1, bad
    assert same_bytes(fx.dihedral_compute(at), want)                     # a refused set_params leaves tables and lists as they were
    # (what is allowed at the edges of those ranges: n = 12 for dihedral harmonic, n = 6 for cvff, a style of 0 with no types)
    assert params(dihedral_style=2, dihedral_coef=dp(cos_rows(ct, 2, 12.0)), improper_style=2, improper_coef=dp(cos_rows(vt, 2, 6.0))) == 0
    assert params(dihedral_style=0, ndihedraltypes=0, dihedral_coef=None) == 0
    assert lists() == -1                                                 # dihedrals for a style that is 0
    assert lists(ndihedral=0, dihedral=None) == 0
    assert fx.dihedral_compute(at)[1][0] == 0.0
    still_fine()
    # set_lists: each refusal leaves the handle without lists, and a valid call gives the unrefused result again
    d_hi, d_neg, d_t0, d_t4 = (c.dihedrals.copy() for _ in range(4))
    d_hi[5, 3] = c.nall; d_neg[7, 0] = -1; d_t0[3, 4] = 0; d_t4[3, 4] = 4
    i_hi, i_neg, i_t0, i_t3 = (c.impropers.copy() for _ in range(4))
    i_hi[2, 2] = c.nall; i_neg[4, 1] = -1; i_t0[1, 4] = 0; i_t3[1, 4] = 3
    nan, inf = float("nan"), float("inf")
    refused = [dict(dihedral=None), dict(improper=None), dict(ndihedral=-1), dict(nimproper=-1), dict(nlocal=-1), dict(nall=-1),
               dict(nlocal=c.nall + 1), dict(dihedral=ip(d_hi)), dict(dihedral=ip(d_neg)), dict(dihedral=ip(d_t0)), dict(dihedral=ip(d_t4)),
               dict(improper=ip(i_hi)), dict(improper=ip(i_neg)), dict(improper=ip(i_t0)), dict(improper=ip(i_t3)),
               dict(prd=(C.c_double * 3)(-1.0, 0, 0)), dict(prd=(C.c_double * 3)(0, nan, 0)), dict(prd=(C.c_double * 3)(0, 0, inf))]
    for bad in refused:
        assert lists(**bad) == -1, bad
        _raises(-2, fx.dihedral_compute, at)
        _raises(-2, fx.dihedral_compute_device, d_x.data_ptr(), 0, 0, 0, 0)
        still_fine()
    assert lib.conp_dihedral_set_lists(fx.h, None) == -1
    _raises(-2, fx.dihedral_compute, at)
    still_fine()
    # the compute entries: NULL d_x / atoms, another atom count
    _raises(-1, fx.dihedral_compute_device, 0, 0, 0, 0, 0)
    assert lib.conp_dihedral_compute(fx.h, None, None, None, None, None, None) == -1
    _raises(-1, fx.dihedral_compute, atoms_of(h))
    short = atoms_of(c); short.nlocal -= 1
    _raises(-1, fx.dihedral_compute, short)
    assert same_bytes(fx.dihedral_compute(at), want)
    # set_params after set_lists drops the lists (they were checked against the old tables)
    set_params(fx, c.p)
    _raises(-2, fx.dihedral_compute, at)
    still_fine()
    # a second set_lists with other lists replaces the first
    fx.dihedral_set_lists(h.nlocal, h.nall, h.dihedrals, h.impropers, h.prd)
    dr.check("other lists", fx.dihedral_compute(atoms_of(h)), dr.for_case(h))
    _raises(-1, fx.dihedral_compute, at)
    still_fine()
    # the bonded entries of the same handle keep their own state
    _raises(-2, fx.bonded_compute, at)
    fx.close()


# ---- the whole device step ----------------------------------------------------------------------------------------------------------
def test_a_whole_step_with_the_dihedral_term():
    """ghost_fill -> pre_force_device -> ewald_forces_device -> pair_compute_device -> bonded_compute_device -> dihedral_compute_device
    -> post_force_device -> ghost_fold_device on one stream with nothing between, on the box and to the bound of
    tests/test_gpu_post_force_device.py's step test: the folded owned forces are the five host entries' sum, folded in numpy"""
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
    # the electrolyte atoms four at a time, where they are: owned indices and the box lengths, handed over once; soft springs and
    # barriers scaled to the distances, so that the terms are of the size of the others.  Of the quadruples those with bond-angle
    # sines of 0.25 or more carry a dihedral and an improper (the condition of the 1e-12 bound, tests/dihedral_ref.py)
    prd = np.where(c.s.periodic, c.s.prd, 0.0)
    x_now = b.d_x.cpu().numpy()[:nall]
    el = np.nonzero(c.own.echeck == 0)[0]
    quad = el[:len(el) // 4 * 4].reshape(-1, 4)
    one = np.ones((len(quad), 1), dtype=int)
    G = dr.reference(x_now, n, np.concatenate([quad, one], 1), None, dr.PARAMS_OPLS, True, prd)
    quad = quad[(G.T.sin1 >= 0.25) & (G.T.sin2 >= 0.25)]
    assert len(quad) >= 8
    one = np.ones(len(quad), dtype=int)
    bonds = np.concatenate([np.stack([quad[:, k], quad[:, k + 1], one], 1) for k in range(3)])
    angles = np.concatenate([np.stack([quad[:, k], quad[:, k + 1], quad[:, k + 2], one], 1) for k in range(2)])
    dihedrals = np.concatenate([quad, one[:, None]], 1)
    impropers = np.concatenate([quad[:, [1, 0, 2, 3]], one[:, None]], 1)
    Gi = dr.reference(x_now, n, None, impropers, dr.PARAMS_OPLS, True, prd)
    impropers = impropers[(Gi.T.sin1 >= 0.25) & (Gi.T.sin2 >= 0.25)]
    soft = SimpleNamespace(bond_k=np.array([0.4]), bond_r0=np.array([3.0]), angle_k=np.array([2.0]), angle_theta0=np.array([1.9]))
    tors = SimpleNamespace(dstyle="opls", dcoef=np.array([[30.0, -12.0, 45.0, 6.0]]), istyle="harmonic", icoef=np.array([[25.0, 0.3]]))
    for fx in (fd, fh):
        fx.bonded_set_params(soft.bond_k, soft.bond_r0, soft.angle_k, soft.angle_theta0, newton_bond=True)
        fx.bonded_set_lists(n, nall, bonds, angles, prd)
        set_params(fx, tors)
        fx.dihedral_set_lists(n, nall, dihedrals, impropers, prd)
    d_f = torch.zeros((nall, 3), dtype=torch.float64, device="cuda")
    d_out = torch.full((9,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    fd.ghost_fill_device(b.d_x.data_ptr(), d_q.data_ptr())
    fd.pre_force_device(b.d_x.data_ptr(), d_q.data_ptr(), c.s.potdiff)
    fd.ewald_forces_device(b.d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), 0, 0)
    fd.pair_compute_device(b.d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), 0, 0, 0)
    fd.bonded_compute_device(b.d_x.data_ptr(), d_f.data_ptr(), 0, 0, 0)
    fd.dihedral_compute_device(b.d_x.data_ptr(), d_f.data_ptr(), 0, 0, 0)
    fd.post_force_device(b.d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), d_out.data_ptr())
    fd.ghost_fold_device(d_f.data_ptr(), 3)
    torch.cuda.synchronize()
    got = d_f.cpu().numpy()[:n]
    at1, lst = tp.host_route(fh, c, fd, b)
    at1.q[:] = d_q.cpu().numpy()[:nall]
    assert at1.x[:n].tobytes() == x_now[:n].tobytes()                    # the terms were chosen on the step's own coordinates
    fh.pair_set_list(lst, nall)
    total = np.zeros((nall, 3))
    total[:n] += fh.ewald_forces(at1, energy=False, virial=False)[0]
    total += fh.pair_compute(at1, eng=False, virial=False, eatom=False, vatom=False)[0]
    total += fh.post_force(at1)[0]
    total += fh.bonded_compute(at1, eng=False, virial=False, eatom=False, vatom=False)[0]
    f_tors = fh.dihedral_compute(at1, eng=False, virial=False, eatom=False, vatom=False)[0]
    assert np.abs(f_tors).max() > 0 and not f_tors[n:].any()            # owned indices: nothing on a ghost row
    R = dr.reference(at1.x, n, dihedrals, impropers, tors, True, prd)
    dr.check("the step's dihedral term, host entry", (f_tors, None, None, None, None), R)
    total += f_tors
    owner = np.asarray(fd.ghost_get()[2], np.int64)
    want = total[:n].copy()
    np.add.at(want, owner, total[n:])
    fr = rel_err(got, want) / tpf.ORACLE
    print(f"a whole step with the dihedral term: fraction of the bound {tpf.ORACLE:g}: force {fr:.3g}")
    assert fr < 1.0
    without = (total - f_tors)[:n].copy()
    np.add.at(without, owner, (total - f_tors)[n:])
    assert rel_err(got, without) > 1e3 * tpf.ORACLE                      # ... and the sum without the term is far outside the bound
    fd.close(); fh.close()
