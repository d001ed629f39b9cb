"""-m gpu: the exact Ewald entries (potential, forces, per-atom virial; host and device forms) at every plan shape, block tier and
size -- DESIGN.md sections 11, 12, 14, 15.  The boxes and the restated host rules are in tests/ewald_shape_cases.py, checked without
a GPU by tests/test_ewald_shape_cases_math.py; every case here first asserts, from the handle and the device's CU count, the tier it
claims, and prints it.

(a) plan shapes: one row tile and K <= 256 (`tiny`), the second half of a column tile (`half2`), two and three column tiles
    (`cols2`, whose outer row tiles leave column tile 1 empty; `cols3`), seven and five row tiles with a ragged last one (`cols2`,
    `wide`), each through the five entries: host potential (group, particle, compute potential/atom), host forces with eatom, host
    forces with vatom, device forces, device forces with vatom;  (b) 1, 63, 64, 65, 129 targets and a probe alone; 127, 128, 129
    charged atoms;  (c) blocks of 64, 128, 192 with a full last block, a last block of one atom, one block for everything, 1, 2 and
    3 splits, all five entries;  (d) uneven splits: 2112 columns over 32 splits of 80, the 27th partial, five empty;  (e) `bigN`:
    66 256 atoms in nine blocks of 8192, kspace_four_sums saturated, a net charge in slab mode;  (f) a net charge of 1 e;
    (g) results do not depend on the calls before them, byte for byte;  (h) guard zones around (b), (c), (d);  (i) a live handle
    re-planned to a smaller plan and back (conp_km_conp_setup) gives what handles set up with either plan give, byte for byte.

References: tests/ewald_force_ref.py, tests/kspace_vatom_ref.py and _brute_g of tests/test_gpu_ewald_potential.py, on ALL owned
atoms (bigN: S over all atoms, per-atom quantities on 512 seeded atoms and the probes).  Bounds, those of the sibling tests and no
others: potential 1e-11 max|g|; forces 1e-10 max|f|; energy, virial, eatom, vatom 1e-11 of qs sum ug |S|^2; sum_i vatom_i against
the call's virial 1e-13 of that scale.

Measured on an MI355X (256 CUs), the largest fraction of each bound over the entries of a case; `pot` is the largest of group
potential, particle potential and potential/atom.  No bound is exceeded, so no float64 floor had to be measured:
    case                          tier                                                   pot     force   energy  virial  eatom   vatom   sum v
    tiny/ffield                   K 59, kzt 8, 1 row tile, nb_pad 192, nsplit 3          1.1e-4  4.0e-6  1.0e-4  2.0e-5  3.6e-5  1.1e-4  2.1e-2
    tiny/slab                     K 83                                                   8.8e-5  7.8e-6  1.9e-4  6.1e-5  4.9e-4  1.3e-4  2.7e-2
    half2/slab                    K 3346, nz 84, kzt 88 (h = 1)                          2.9e-4  1.6e-5  2.3e-5  1.5e-5  7.5e-5  4.5e-5  7.5e-3
    half2/ffield                                                                         1.2e-4  1.5e-5  2.2e-5  6.6e-5  9.6e-6  3.2e-5  4.4e-3
    cols2/slab                    K 107163, nz 168, 2 column tiles, kzt 88, 7 row tiles  1.8e-4  1.6e-5  3.2e-5  2.6e-5  1.0e-5  2.6e-5  1.9e-3
    cols2/ffield                  (np 405: last tile ragged; outer 64 reach kz 81 < kzt)  2.1e-4  1.7e-5  2.3e-5  7.5e-6  1.6e-5  2.5e-5  4.5e-3
    cols3/slab                    K 32078, nz 348, 3 column tiles, kzt 120, 128 atoms    1.5e-4  5.7e-5  4.4e-5  4.4e-5  1.6e-5  3.9e-5  1.0e-2
    cols3/ffield                                                                         1.7e-4  4.0e-5  1.5e-5  4.4e-5  1.6e-5  6.8e-5  4.4e-3
    wide/ffield                   K 9483, np 260: 5 row tiles, nb_pad 320, nsplit 5      5.3e-5  1.0e-5  0       2.7e-5  8.7e-6  1.4e-5  6.7e-4
    (b) 127 / 128 / 129 charged   host nb_pad 128 / 128 / 192, device 192 (worst)        -       7.0e-6  2.7e-4  1.5e-4  5.0e-5  9.9e-5  1.8e-2
    (b) 1, 63, 64, 65, 129 targets, a probe alone: group potential 1.1e-4 at most
    (c) six block cases           widths 64 / 128 / 192, nsplit 1 / 2 / 3 (worst)        1.7e-4  1.3e-5  8.7e-5  5.8e-5  8.0e-5  1.6e-4  9.7e-3
    (d) uneven/slab               nb_pad 2112, nsplit 32, per_split 80, 27th partial,    3.8e-3  5.2e-5  4.6e-4  4.2e-4  1.5e-4  1.0e-4  7.0e-3
                                  5 empty splits
    (e) bigN/slab Q = +1          66256 atoms, K 1549, 9 blocks of 8192 (last 720 /      2.1e-3  4.0e-5  2.9e-4  3.1e-4  9.0e-6  6.7e-6  5.2e-3
                                  716), nsplit 32, per_split 256, four sums saturated
    (f) tiny/ffield Q = +1                                                               4.8e-5  4.8e-6  3.7e-4  7.8e-5  1.6e-5  3.3e-5  8.2e-3
    (f) half2/slab Q = +1                                                                2.0e-4  1.4e-5  8.8e-5  5.4e-5  7.8e-5  4.9e-5  1.1e-2
    (g) byte-identical to fresh handles; (h) no guard zone damaged; (i) byte-identical to handles set up with either plan (tiny/slab,
    K 83 -> 5 -> 83).  The 27 tests take 20 s.
The finding of (e): with the host entries' four sums and the potential/atom tail added in plain loops, bigN's host entries stood at
0.84 (potential/atom), 0.11 (energy), 0.059 (force) and 0.028 (eatom) of their bounds -- 66 000 sites sharing four charge values lose
1e-8 of Q in a running sum -- where the device entries' tree sums gave 3e-4 and less.  The library now adds them with a compensated
sum (CompSum, conp_kspace_common.hpp); the row above is measured with it."""
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import ewald_force_ref as eref
import ewald_shape_cases as sc
import kspace_vatom_ref as vref
from conp_amd import FixConp, capi, systems
from test_gpu_ewald_potential import EVS, _add_probes, _brute_g
from test_gpu_kspace_device import _call, _to_device
from test_gpu_kspace_vatom import _vcall

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("potential", "host_eatom", "host_vatom", "device", "device_vatom")
FRACTIONS = {}                                   # case tag -> {quantity: largest fraction of its bound}


def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _compare(tag, what, got, want, bound):
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    frac = err / bound
    row = FRACTIONS.setdefault(tag.split(" [")[0], {})            # (the largest over the entries of a case)
    row[what] = max(row.get(what, 0.0), frac)
    print(f"{tag} {what}: max error {err:.3e}, bound {bound:.3e} ({frac:.3g} of it)")
    assert err <= bound, (tag, what, err, bound)


def _handle(s, update=True):
    at, alist, blist = sc.build_atoms(s)
    fx = FixConp(s)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    if update:
        fx.setup_pre_force(at, 0, s.potdiff)         # electrode atoms carry their solved charges from here on
        fx.pre_force(at, 1, s.potdiff)
    else:
        sc.seed_electrode_charges(at)
    return at, alist, blist, fx


def _potential_from_S(S, x, kv, ug, targets, chunk=512):
    """_brute_g's second half at a structure factor that is already there (bigN forms its one O(N K) sum once)"""
    g = np.zeros(len(targets))
    for a in range(0, len(targets), chunk):
        ph = x[targets[a:a + chunk]] @ kv.T
        g[a:a + chunk] = -(2 * ug * (np.cos(ph) * S.real + np.sin(ph) * S.imag)).sum(axis=1)
    return g


@functools.lru_cache(maxsize=None)
def case(name, mode, net=0.0, charged=None):
    """a handle after an update, probes added, [a net charge], [charges zeroed down to `charged`], the atoms on the device and the
    numpy references at them: formed once per process and never changed"""
    s = sc.system(name, mode)
    big = name == "bigN"
    at, alist, blist, fx = _handle(s, update=not big)
    n = at.nlocal
    probes = _add_probes(s, at)
    if net:
        sc.shift_net_charge(at, net)
    if charged is not None:
        sc.zero_charges_to(at, charged)
    x, q = np.ascontiguousarray(at.x[:n]), np.ascontiguousarray(at.q[:n])
    if big:
        rng = np.random.default_rng(3)
        tg = np.concatenate([np.sort(rng.choice(np.setdiff1d(np.arange(n), probes), 512, replace=False)), probes])
    else:
        tg = np.arange(n)
    T = eref.handle_tables(fx, s)
    S = eref.structure_factor(x, q, T["kv"])
    E, W = eref.energy_virial(S, x, q, T["kv"], T["ug"], T["g"], T["V"], T["qs"], T["slab"], T["L"])
    f, e = eref.forces_eatom(S, x, q, T["kv"], T["ug"], T["g"], T["V"], T["qs"], tg, T["slab"], T["L"])
    v = vref.ewald_vatom(S, x, q, T["kv"], T["ug"], T["g"], T["qs"], tg)
    g = _potential_from_S(S, x, T["kv"], T["ug"], tg) if big else _brute_g(fx, at, tg)
    d_x, d_q = _to_device(at)
    tag = f"{name}/{mode}" + (f" Q={q.sum():+.2f}" if net else "") + (f" {charged} charged" if charged is not None else "")
    return SimpleNamespace(s=s, at=at, alist=alist, blist=blist, fx=fx, n=n, probes=probes, x=x, q=q, tg=tg, T=T, S=S, E=E, W=W, f=f, e=e,
                           v=v, g=g, scale=T["qs"] * eref.ksum(S, T["ug"]), d_x=d_x, d_q=d_q, tag=tag, sh=sc.handle_shape(fx),
                           n_charged=int((q != 0).sum()), zero=np.nonzero(q == 0)[0])


def tiers(c, width=0):
    """the tiers of a call on case c, asserted against nothing yet: (host entries' force blocks and columns, device entries')"""
    cus = _cus()
    th, td = sc.tier(c.sh, c.n_charged, cus, width), sc.tier(c.sh, c.n, cus, width)
    print(f"{c.tag}: {cus} CUs, K {c.sh['K']}; host entries ({c.n_charged} charged): {sc.describe(th)}; "
          f"device entries ({c.n} owned): {sc.describe(td)}")
    return th, td


# ---- the five entries against the references -------------------------------------------------------------------------------
def _check_forces(c, tag, gf, gE, gW, ge, gv):
    """the outputs of a force entry on all owned atoms against the case's references at c.tg"""
    assert np.abs(c.f).max() > 0 and c.scale > 0
    assert np.all(gf[c.zero] == 0.0) and np.all(ge[c.zero] == 0.0)           # zero charges: exact zeros
    _compare(tag, "force", gf[c.tg], c.f, 1e-10 * np.abs(c.f).max())
    _compare(tag, "energy", gE, c.E, 1e-11 * c.scale)
    _compare(tag, "virial", gW, c.W, 1e-11 * c.scale)
    _compare(tag, "eatom", ge[c.tg], c.e, 1e-11 * c.scale)
    if gv is not None:
        assert gv.shape == (c.n, 6) and np.all(np.isfinite(gv)) and np.all(gv[c.zero] == 0.0) and np.abs(c.v).max() > 0
        _compare(tag, "vatom", gv[c.tg], c.v, 1e-11 * c.scale)
        # (each component as one contiguous row: numpy adds those pairwise, rows of [n][6] one after the other)
        _compare(tag, "sum vatom", np.ascontiguousarray(gv.T).sum(axis=1), gW, 1e-13 * c.scale)


def run_potential(c, tag, sel_idx=None, particles=True):
    """the host potential entry: group_potential on a seeded half of the atoms (or sel_idx), particle_potential on a few,
    compute_potential_atom(pair=False, kspace=True)"""
    at, fx, n, s = c.at, c.fx, c.n, c.s
    pos = {int(i): k for k, i in enumerate(c.tg)}                 # atom -> its row of the references
    if sel_idx is None:
        pick = c.tg[np.random.default_rng(11).random(len(c.tg)) < 0.5]
        sel_idx = np.unique(np.concatenate([pick, c.probes, np.nonzero(at.echeck[:n] != 0)[0][:7]]))
        sel_idx = np.array([i for i in sel_idx if int(i) in pos])
    sel = np.zeros(n, np.int32)
    sel[sel_idx] = 1
    rows = np.array([pos[int(i)] for i in sel_idx])
    want = c.g[rows]
    gscale = np.abs(c.g).max()
    fx.ewald_compute(at)                               # S of THESE atoms (the probes were made after the handle's update)
    got = fx.ewald_group_potential(at, sel)
    assert np.all(got[sel == 0] == 0.0)
    _compare(tag, "group potential", got[sel_idx], want, 1e-11 * gscale)
    if not particles:
        return
    some = list(range(0, len(sel_idx), max(1, len(sel_idx) // 5))) + [k for k, i in enumerate(sel_idx) if i in c.probes]
    u = np.array([fx.ewald_particle_potential(at, int(sel_idx[k])) for k in some])
    _compare(tag, "particle potential", u, want[some] + 2 * s.g_ewald * c.q[sel_idx[some]] / np.sqrt(np.pi), 1e-11 * gscale)
    nall = at.nlocal + at.nghost
    sel_all = np.zeros(nall, np.int32)
    sel_all[:n] = sel
    pot = fx.compute_potential_atom(at, c.blist, sel_all, pair=False, kspace=True, qsum=True)
    ref = -(want + 2 * s.g_ewald * c.q[sel_idx] / np.sqrt(np.pi))
    if s.slabflag:
        pi2vol = 2 * np.pi / c.T["V"]
        z = c.x[:, 2]
        ref = ref + z[sel_idx] * (2 * pi2vol * c.q * z).sum() - pi2vol * c.q.sum() * z[sel_idx] ** 2
    _compare(tag, "potential/atom", pot[sel_idx], EVS * ref, 1e-11 * EVS * np.abs(ref).max())


def run_host_forces(c, tag, vatom):
    c.fx.ewald_compute(c.at)
    if vatom:
        f, E, W, e, v = c.fx.ewald_forces_vatom(c.at, eatom=True)
    else:
        (f, E, W, e), v = c.fx.ewald_forces(c.at, eatom=True), None
    _check_forces(c, tag, f, E, W, e, v)


def run_device_forces(c, tag, vatom):
    if vatom:
        f, ev, e, v = _vcall(c.fx.ewald_forces_vatom_device, c.d_x, c.d_q, c.n)
    else:
        (f, ev, e), v = _call(c.fx.ewald_forces_device, c.d_x, c.d_q, c.n), None
    _check_forces(c, tag, f, ev[0], ev[1:], e, v)


def run_entries(c, label="", entries=ENTRIES):
    for entry in entries:
        tag = f"{c.tag}{label} [{entry}]"
        if entry == "potential":
            run_potential(c, tag)
        elif entry.startswith("host"):
            run_host_forces(c, tag, entry == "host_vatom")
        else:
            run_device_forces(c, tag, entry == "device_vatom")


# ---- (a) plan shapes -------------------------------------------------------------------------------------------------------
def run_plan_shape(name, mode):
    c = case(name, mode)
    th, td = tiers(c)
    sc.check_declared_shape(name, c.sh, c.n, c.n_charged, _cus())
    assert th["blocks"] == td["blocks"] == 1                      # (blocks are cases (c) and (e))
    run_entries(c)


@pytest.mark.parametrize("name,mode", sc.SMALL_CASES)
def test_every_plan_shape(name, mode):
    run_plan_shape(name, mode)


# ---- (b) target and atom counts --------------------------------------------------------------------------------------------
def run_target_counts():
    c = case(*sc.B_BOX)
    tiers(c)
    rng = np.random.default_rng(23)
    charged = np.setdiff1d(np.arange(c.n), c.zero)
    for m in sc.B_TARGETS:
        sel_idx = np.sort(np.concatenate([rng.choice(charged, m - 1, replace=False), c.probes[:1]]))     # (a probe is always among them)
        t = sc.tier(c.sh, m, _cus())
        print(f"{c.tag}: {m} target(s): {sc.describe(t)}")
        assert len(sel_idx) == m and t["nb_pad"] == min(192, (m + 63) // 64 * 64)
        run_potential(c, f"{c.tag} [{m} targets]", sel_idx, particles=False)
    run_potential(c, f"{c.tag} [a probe alone]", c.probes[1:2], particles=False)


def test_potential_with_1_63_64_65_129_targets_and_a_probe_alone():
    run_target_counts()


def run_charged_count(charged):
    c = case(*sc.B_BOX, charged=charged)
    th, td = tiers(c)
    assert c.n_charged == charged and th["nb_pad"] == (charged + 63) // 64 * 64 and td["nb_pad"] == 192
    assert len(c.zero) == c.n - charged > len(c.probes)
    run_entries(c, entries=ENTRIES[1:])


@pytest.mark.parametrize("charged", sc.B_CHARGED)
def test_forces_with_127_128_129_charged_atoms(charged):
    run_charged_count(charged)


# ---- (c) blocks ------------------------------------------------------------------------------------------------------------
def run_blocks(box, width, charged):
    want = sc.C_CASES[(box, width, charged)]
    c = case(box, "slab", charged=charged)
    capi.set_ew_block(width)
    try:
        th, td = tiers(c, width)
        assert sc.situation(th) == want["host"] and sc.situation(td) == want["device"], (th, td)
        assert th["nsplit"] == want["nsplit"] and th["per_split"] == 64, th
        run_entries(c, f", blocks of {width}")
    finally:
        capi.set_ew_block(0)


def test_block_cases_cover_every_situation():
    hosts = {w["host"] for w in sc.C_CASES.values()}
    devices = {w["device"] for w in sc.C_CASES.values()}
    assert hosts == {"full", "one", "single"} and devices >= {"full", "one", "single"}
    assert {w["nsplit"] for w in sc.C_CASES.values()} == {1, 2, 3}


@pytest.mark.parametrize("box,width,charged", list(sc.C_CASES))
def test_all_entries_in_blocks(box, width, charged):
    run_blocks(box, width, charged)


# ---- (d) uneven splits -----------------------------------------------------------------------------------------------------
def run_uneven_splits():
    c = case(*sc.D_BOX)
    th, td = tiers(c)
    sc.check_declared_shape("uneven", c.sh, c.n, c.n_charged, _cus())
    for t in (th, td):
        assert t["blocks"] == 1 and t["nb_pad"] % (t["nsplit"] * 16) != 0 and t["empty_splits"] >= 1, t
        if _cus() == sc.CUS:
            assert (t["nb_pad"], t["nsplit"], t["per_split"], t["splits_used"], t["partial"], t["empty_splits"]) == (2112, 32, 80, 27, 32, 5)
    run_entries(c, entries=("potential", "host_eatom", "device_vatom"))


def test_uneven_splits_with_a_partial_and_empty_trailing_splits():
    run_uneven_splits()


# ---- (e) bigN --------------------------------------------------------------------------------------------------------------
def test_more_than_65536_atoms_in_blocks_of_8192():
    c = case("bigN", "slab", net=1.0)
    th, td = tiers(c)
    sc.check_declared_shape("bigN", c.sh, c.n, c.n_charged, _cus())
    for t in (th, td):
        assert t["nb_pad"] == 8192 and t["blocks"] >= 9 and 0 < t["last"] < 8192, t
    assert sc.four_sums_workgroups(c.n) == 256 and c.n > 65536 and c.s.slabflag and abs(c.q.sum()) > 0.5
    run_device_forces(c, f"{c.tag} [device_vatom]", True)
    run_host_forces(c, f"{c.tag} [host_eatom]", False)
    run_potential(c, f"{c.tag} [potential]", c.tg)


# ---- (f) net charge --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", sc.F_BOXES)
def test_a_net_charge(name, mode):
    c = case(name, mode, net=1.0)
    tiers(c)
    assert abs(c.q.sum()) > 0.5 and {m for _, m in sc.F_BOXES} == {"ffield", "slab"}
    run_entries(c)


# ---- (g) independence of earlier calls -------------------------------------------------------------------------------------
def test_results_do_not_depend_on_the_calls_before_them():
    """no atomics and a fixed summation order: byte identity with a fresh handle is the contract"""
    c = case(*sc.G_BOX)
    at, n = c.at, c.n

    def fresh():
        fx = _handle(c.s)[3]
        return fx

    def potential_all(fx):
        fx.ewald_compute(at)
        return fx.ewald_group_potential(at, np.ones(n, np.int32))

    def device(fx):
        return _call(fx.ewald_forces_device, c.d_x, c.d_q, n)

    fx = fresh()
    sel5 = np.zeros(n, np.int32)
    sel5[[0, 3, n // 2, n - 2, n - 1]] = 1
    try:
        fx.ewald_compute(at)
        fx.ewald_group_potential(at, sel5)                                        # 1
        device(fx)                                                                # 2
        capi.set_ew_block(64)
        fx.ewald_compute(at)
        fx.ewald_forces(at, eatom=True)                                           # 3
        capi.set_ew_block(128)
        _vcall(fx.ewald_forces_vatom_device, c.d_x, c.d_q, n)                     # 4
        capi.set_ew_block(0)
        g5 = potential_all(fx)                                                    # 5
        out6 = device(fx)                                                         # 6
    finally:
        capi.set_ew_block(0)
    fa, fb = fresh(), fresh()
    g5_fresh, out6_fresh = potential_all(fa), device(fb)
    _compare(c.tag, "group potential after the sequence", g5, c.g, 1e-11 * np.abs(c.g).max())        # (and it is right)
    assert g5.tobytes() == g5_fresh.tobytes(), np.abs(g5 - g5_fresh).max()
    for name, a, b in zip(("f", "ev", "eatom"), out6, out6_fresh):
        assert a.tobytes() == b.tobytes(), (name, np.abs(a - b).max())
    for h in (fx, fa, fb):
        h.close()


# ---- (i) re-planning a live handle -----------------------------------------------------------------------------------------
def test_replanned_handle_gives_what_a_fresh_handle_of_that_plan_gives():
    """The smaller plan inside buffers sized and zeroed for the larger one: stale padding rows of the phase tables, a stale k list
    or stale tile lists would show.  Byte identity with handles that never had another plan is the contract."""
    c = case(*sc.I_BOX)
    at, n, s = c.at, c.n, c.s
    sB = sc.with_qsqsum_factor(s, sc.I_QSQ_FACTOR)
    qsq_A, qsq_B = s.qsqsum, sB.qsqsum

    def four_calls(fx):
        fx.ewald_compute(at)
        g = fx.ewald_group_potential(at, np.ones(n, np.int32))
        f, E, W, e = fx.ewald_forces(at, eatom=True)
        return (g, f, np.float64(E), W, e) + tuple(_vcall(fx.ewald_forces_vatom_device, c.d_x, c.d_q, n))

    def plan(fx):
        sh, kt = sc.handle_shape(fx), fx.ktables()
        assert sh["K"] == fx.info().kcount
        return sh, np.stack([kt["kxvecs"], kt["kyvecs"], kt["kzvecs"]]).tobytes() + kt["ug"].tobytes()

    H = _handle(s)[3]
    pA = plan(H)
    four_calls(H)                                                                 # first round, plan A
    H.km_conp_setup(qsq_B, s.natoms)
    pB = plan(H)
    a, b = pA[0], pB[0]
    print(f"{c.tag}: plan A {a}\n{c.tag}: plan B {b}")
    assert b["K"] < a["K"] and b["np"] < a["np"] and b["nz"] < a["nz"] and b["kxmax"] < a["kxmax"] and b["kymax"] < a["kymax"]
    assert (b["R_pad"], b["C_pad"]) == (a["R_pad"], a["C_pad"])                   # B lies inside A's buffers
    second = four_calls(H)
    H.km_conp_setup(qsq_A, s.natoms)
    assert plan(H) == pA
    third = four_calls(H)
    # the fresh handles: set up with the atoms whose sum q^2 gives the plan (no update: the entries read the charges of the call)
    FB, FA = _handle(sB, update=False)[3], _handle(s, update=False)[3]
    assert plan(FB) == pB and plan(FA) == pA
    names = ("group potential", "f", "E", "W", "eatom", "device f", "device ev", "device eatom", "device vatom")
    for label, got, fresh in (("second round against plan B", second, four_calls(FB)), ("third round against plan A", third, four_calls(FA))):
        assert len(got) == len(fresh) == len(names)
        for name, x, y in zip(names, got, fresh):
            assert np.abs(y).max() > 0 and x.tobytes() == y.tobytes(), (label, name, np.abs(x - y).max())
    assert any(x.tobytes() != y.tobytes() for x, y in zip(second, third))          # (the two plans do give different numbers)
    _compare(c.tag, "group potential after the re-plans", third[0], c.g, 1e-11 * np.abs(c.g).max())      # (and plan A's are right)
    for h in (H, FB, FA):
        h.close()


# ---- (h) guard zones -------------------------------------------------------------------------------------------------------
CHILD = r'''
import sys
sys.path[:0] = [{tests!r}, {pkg!r}, {oracle!r}, {root!r}]
import torch
torch.cuda.init()
import ewald_shape_cases as sc
import test_gpu_ewald_shapes as t
from conp_amd import capi
lib = capi.load_library()
lib.conp_debug_check_guards.restype = int
assert lib.conp_debug_check_guards() == 0, "guard zones are off"
t.run_target_counts()
for charged in sc.B_CHARGED:
    t.run_charged_count(charged)
for box, width, charged in sc.C_CASES:
    t.run_blocks(box, width, charged)
t.run_uneven_splits()
bad = lib.conp_debug_check_guards()
assert bad == 0, (bad, lib.conp_last_error().decode())
print("GUARD_OK")
'''


def test_no_store_outside_the_buffers(tmp_path):
    script = tmp_path / "guard_child.py"
    script.write_text(CHILD.format(tests=os.path.join(ROOT, "tests"), pkg=os.path.join(ROOT, "lammps-user-conp2_amd"),
                                   oracle=os.path.join(ROOT, "oracle"), root=ROOT))
    env = dict(os.environ, CONP_GUARD="1")
    p = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "GUARD_OK" in p.stdout


def teardown_module(module):
    """the table of the module docstring: the largest fraction of each bound per case"""
    cols = ("group potential", "particle potential", "potential/atom", "force", "energy", "virial", "eatom", "vatom", "sum vatom")
    print("\n" + " | ".join(("case",) + cols))
    for tag, row in FRACTIONS.items():
        print(" | ".join([tag] + [f"{row[k]:.2g}" if k in row else "-" for k in cols]))
