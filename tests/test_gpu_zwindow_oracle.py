"""-m gpu: the z-window form of the structure-factor contraction (conp_zn.hip) against the CPU oracle and numpy, at its edges.

tests/test_gpu_zwindow.py compares the z-window path with the same library's full kernels (CONP_PATH_SK_CLASSIC); a fault the two
share (phase tables, k plan, weights, projection) passes there.  Here every case is compared with the oracle's FP64 restatement of
the reference loops (S(k) from sincos_b, b from ele_trig + bbb + blist) or with numpy, and first asserts the path it claims to test:
zn_cols (32 / 48, or 0 where the code falls back), zn_grid (the planned grid, from the k plan on the host) and n_zclasses.

Charges: the oracle's A matrix at these sizes takes hours, so the electrode charges are checked as  q = S b_oracle + dV S d  with S
and S d from the handle (fx.matrix(), the setq of fx.vectors()); S itself is pinned against A at the headline size by
tests/test_gpu_decks.py::test_headline_inverse_really_inverts.  Bars: S(k) and b 1e-11 of the largest entry,
charges 1e-8 relative."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conp_amd import FixConp, capi, neighbor, systems
from helpers import oracle_sk_and_b, rel_err, sk_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SK_BAR, B_BAR, Q_BAR = 1e-11, 1e-11, 1e-8


def _medium(mode="ffield", seed=7, **kw):
    a = dict(n_cells_x=16, n_cells_y=8, lz=300.0, n_elyte=16384, cutoff=12.0, accuracy_relative=1e-6, g_ewald=0.26, mode=mode,
             seed=seed)
    a.update(kw)
    return systems.synthetic_fast(**a)


def _rough(mode):
    s = _medium(mode, seed=23)
    ele = s.echeck != 0
    s.x[ele, 2] += np.random.default_rng(23).uniform(-0.4, 0.4, size=int(ele.sum()))      # every electrode atom its own z
    return s


def _nine_classes():
    """layers=4 (8 sheets, the SK_HC_MAX limit) with half of one outer sheet lifted by 1 A: 9 distinct electrode z values"""
    s = _medium(layers=4, seed=31)
    sheet = np.nonzero(s.echeck == 1)[0]
    outer = sheet[s.x[sheet, 2] < s.x[sheet, 2].min() + 0.1]
    s.x[outer[: len(outer) // 2], 2] += 1.0
    return s


def _smallest_grid():
    """the grid floor: nz = 11 (lz 60 A, accuracy 1e-4, g_ewald 0.2) plans n = max(64, 48) = 64 with 16384 charged atoms"""
    return _medium(lz=60.0, accuracy_relative=1e-4, g_ewald=0.2, seed=13)


def _vapour_gap():
    """two electrolyte compartments: the charges of the liquid within 40 A of the mid-plane are switched off (a vapour gap), so
    the charged list has two empty runs in z -- the 80 A gap, which zn_order_list skips, and the 36 A around the electrodes"""
    s = _medium(seed=37)
    s.q[(s.echeck == 0) & (np.abs(s.x[:, 2]) < 40.0)] = 0.0
    return s


CASES = {
    "smallest_grid": _smallest_grid,
    "headline_slab": lambda: systems.synthetic_fast(mode="slab"),
    "medium_layers2": lambda: _medium(layers=2, seed=41),
    "medium_layers4": lambda: _medium(layers=4, seed=43),
    "rough_ffield": lambda: _rough("ffield"),
    "rough_slab": lambda: _rough("slab"),
}


def _zn_grid(s):
    from test_zwindow_math import zn_grid_of
    return zn_grid_of(s)


def assert_path(fx, s, cols, nzc):
    """the handle took the path the case claims: zn_cols (a tuple of allowed values), the planned z grid, the z classes"""
    info = fx.info()
    assert info.zn_cols in cols, (info.zn_cols, cols)
    if info.zn_cols:
        assert info.zn_grid == _zn_grid(s), (info.zn_grid, _zn_grid(s))
    assert info.n_zclasses == nzc, (info.n_zclasses, nzc)
    return info


def check_sk_b(fx, s, at, alist, blist, label):
    """S(k) and b of the handle's last b_cal against the oracle's at the atoms as they are; returns b_oracle"""
    sr, si, b_o, ks = oracle_sk_and_b(s, at, alist, blist)
    ks.close()
    sr_g, si_g = fx.sfac()
    b_g = fx.vectors()[0]
    e_s, e_b = sk_err(sr_g, si_g, sr, si), rel_err(b_g, b_o)
    print(f"{label}: zn_cols {fx.info().zn_cols} zn_grid {fx.info().zn_grid} nzc {fx.info().n_zclasses}: "
          f"S(k) {e_s:.2e}, b {e_b:.2e} of max")
    assert e_s < SK_BAR, (label, e_s)
    assert e_b < B_BAR, (label, e_b)
    return b_o


def check_charges(fx, s, at, q_atoms, b_o, label, potdiff=None):
    """electrode charges of the last update against S b_oracle + dV S d; electrolyte charges untouched, bit for bit"""
    potdiff = s.potdiff if potdiff is None else potdiff
    S = fx.matrix()
    setq = fx.vectors()[2]
    want = S @ b_o + potdiff * setq
    m = fx.maps()
    loc = {int(t): i for i, t in enumerate(at.tag[:at.nlocal])}
    qe = np.array([q_atoms[loc[int(t)]] for t in m["eleall2tag"]])
    e_q = rel_err(qe, want)
    print(f"{label}: charges {e_q:.2e} relative")
    assert e_q < Q_BAR, (label, e_q)
    sol = at.echeck == 0
    assert np.array_equal(q_atoms[sol], at.q[sol])


def _handle(s, at, alist, blist, linalg=False):
    fx = FixConp(s)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    if linalg:
        fx.linalg_setup(at)
    return fx


def _update(fx, s, at):
    """one host-buffer update at the atoms as they are: returns the charges it wrote (at.q itself is left as it was)"""
    q_in = at.q.copy()
    fx.pre_force(at, 1, s.potdiff)
    q_out = at.q.copy()
    at.q[:] = q_in
    return q_out


# ---- several z classes, off the projecting path, rough electrodes, 48 columns, the smallest grid -------------------------------
@pytest.mark.parametrize("name,nzc,charges", [
    ("medium_layers2", 4, True),
    ("medium_layers4", 8, True),               # SK_HC_MAX
    ("smallest_grid", 2, False),
])
def test_planar_z_window_matches_the_oracle(name, nzc, charges):
    """several z classes in zn_ptable, the pieces and b_zc; the grid floor n = 64.  The smallest grid the planner can produce is
    64 = 2 x 32 columns, so no grid narrower than twice the window is reachable with 32 columns: this case guards the rint fold
    of the window row (conp_kernels.hip) for a later change of the grid rule."""
    s = CASES[name]()
    at, alist, blist = neighbor.build_lists(s)
    fx = _handle(s, at, alist, blist, linalg=charges)
    fx.b_cal(at)                                         # (the z classes are known from the first b_cal / a_cal on)
    info = assert_path(fx, s, (32, 48), nzc)
    if name == "smallest_grid":
        assert info.zn_grid == 64 and info.n_elyte_charged >= 8192
    b_o = check_sk_b(fx, s, at, alist, blist, name)
    if charges:
        q = _update(fx, s, at)
        assert fx.info().zn_cols in (32, 48)
        check_charges(fx, s, at, q, b_o, name)
    fx.close()


def test_nine_z_classes_leave_the_projecting_path():
    """nine classes (one more than SK_HC_MAX): sk_projects() is false and the z-window needs nzc == 0 for its general form, so the
    handle runs the full kernels (zn_cols == 0) -- and b is still the oracle's"""
    s = _nine_classes()
    at, alist, blist = neighbor.build_lists(s)
    fx = _handle(s, at, alist, blist)
    fx.b_cal(at)
    assert_path(fx, s, (0,), 9)
    check_sk_b(fx, s, at, alist, blist, "nine classes")
    fx.close()


@pytest.mark.parametrize("mode", ["ffield", "slab"])
def test_rough_z_window_matches_the_oracle(mode):
    """rough electrodes: zn_gemm<RAW> -> zn_wsum -> zn_dft -> the general projection"""
    s = CASES["rough_" + mode]()
    at, alist, blist = neighbor.build_lists(s)
    fx = _handle(s, at, alist, blist)
    fx.b_cal(at)
    assert_path(fx, s, (32, 48), 0)
    check_sk_b(fx, s, at, alist, blist, "rough " + mode)
    fx.close()


@pytest.mark.parametrize("rough", [False, True])
def test_48_window_columns_match_the_oracle(rough):
    """NCF = 3 of both template forms (planar projection and rough raw windows).  At the medium size the planner takes 32 columns
    (a range of >= 96 atoms would have to span >= 14 grid cells, a liquid ~20 times thinner), so CONP_PATH_ZN_WIDE asks for 48
    wherever 48 do"""
    s = _rough("ffield") if rough else _medium(seed=47)
    at, alist, blist = neighbor.build_lists(s)
    with capi.test_paths(capi.PATH_ZN_WIDE):
        fx = _handle(s, at, alist, blist, linalg=not rough)
        fx.b_cal(at)
        assert_path(fx, s, (48,), 0 if rough else 2)
        b_o = check_sk_b(fx, s, at, alist, blist, f"48 columns rough={rough}")
        if not rough:
            q = _update(fx, s, at)
            assert fx.info().zn_cols == 48
            check_charges(fx, s, at, q, b_o, "48 columns")
        fx.close()


# ---- motion between list builds ------------------------------------------------------------------------------------------------
def test_drift_just_inside_the_margin_matches_the_oracle():
    """every owned electrolyte atom drifts by up to +-2.4 A in z (ZN_DRIFT = 2.5), its ghost images with it: no overflow, the
    window path stays on, S(k), b and the charges are the oracle's at the new positions"""
    s = _medium(seed=53)
    at, alist, blist = neighbor.build_lists(s)
    fx = _handle(s, at, alist, blist, linalg=True)
    assert_path(fx, s, (32, 48), 2)
    fx.mesg_drain()
    dz = np.zeros(at.nlocal)
    sol = at.echeck[:at.nlocal] == 0
    dz[sol] = np.random.default_rng(53).uniform(-2.4, 2.4, size=int(sol.sum()))
    at.x[:, 2] += dz[at.owner]
    q = _update(fx, s, at)
    assert "z-window" not in fx.mesg_drain()
    assert fx.info().zn_cols in (32, 48)
    b_o = check_sk_b(fx, s, at, alist, blist, "drift 2.4 A")
    check_charges(fx, s, at, q, b_o, "drift 2.4 A")
    fx.close()


def test_atoms_moved_across_the_periodic_z_boundary_match_the_oracle():
    """the box of test_z_window_ragged_list_across_the_periodic_wrap (liquid straddling the z boundary, a ragged list); atoms within
    1 A of the boundary then cross it by 0.8 A and are NOT wrapped back: the window row folds them onto the grid"""
    s = _medium(seed=19)
    lo, hi = s.boxlo[2], s.boxlo[2] + s.prd[2]
    s.x[:, 2] = lo + np.mod(s.x[:, 2] - lo + 0.37 * s.prd[2], s.prd[2])
    sol = np.nonzero((s.echeck == 0) & (s.q != 0))[0]
    s.q[sol[[3, 500, 7001, 7002, 16000]]] = 0.0
    at, alist, blist = neighbor.build_lists(s)
    fx = _handle(s, at, alist, blist)
    fx.b_cal(at)
    assert_path(fx, s, (32, 48), 2)
    fx.mesg_drain()
    z = at.x[:at.nlocal, 2]
    liq = at.echeck[:at.nlocal] == 0
    up, down = liq & (z > hi - 1.0), liq & (z < lo + 1.0)
    assert up.sum() > 10 and down.sum() > 10
    dz = np.where(up, 0.8, 0.0) - np.where(down, 0.8, 0.0)
    at.x[:, 2] += dz[at.owner]
    assert at.x[:at.nlocal, 2].max() > hi and at.x[:at.nlocal, 2].min() < lo
    fx.b_cal(at)
    assert fx.info().zn_cols in (32, 48)
    check_sk_b(fx, s, at, alist, blist, "across the z boundary")
    fx.close()


def test_overflow_in_pre_force_then_post_neighbor_matches_the_oracle():
    """an atom jumps 60 A: the host-buffer update notices and repeats itself on the full kernels (charges = oracle's); the
    re-neighbouring at the new positions turns the window back on, and b and the charges are the oracle's again"""
    s = _medium(seed=59)
    at, alist, blist = neighbor.build_lists(s)
    fx = _handle(s, at, alist, blist, linalg=True)
    assert_path(fx, s, (32, 48), 2)
    fx.mesg_drain()
    j = int(np.nonzero((at.echeck[:at.nlocal] == 0) & (at.q[:at.nlocal] != 0))[0][17])
    at.x[at.owner == j, 2] += 60.0
    q = _update(fx, s, at)
    assert "z-window" in fx.mesg_drain() and fx.info().zn_cols == 0
    b_o = check_sk_b(fx, s, at, alist, blist, "overflow, repeated update")
    check_charges(fx, s, at, q, b_o, "overflow, repeated update")
    fx.post_neighbor(at)
    assert_path(fx, s, (32, 48), 2)
    q = _update(fx, s, at)
    assert fx.info().zn_cols in (32, 48) and "z-window" not in fx.mesg_drain()
    b_o = check_sk_b(fx, s, at, alist, blist, "after the re-neighbour")
    check_charges(fx, s, at, q, b_o, "after the re-neighbour")
    fx.close()


def test_charges_switched_between_list_builds_match_the_oracle():
    """one electrolyte charge switched on and one off after the list build (atoms drifted 1 A meanwhile): b_cal rebuilds and
    re-sorts the list at the current positions, on the window path"""
    s = _medium(seed=61)
    sol = np.nonzero(s.echeck == 0)[0]
    off, on = sol[100], sol[9000]
    q_on = s.q[on]
    s.q[on] = 0.0
    at, alist, blist = neighbor.build_lists(s)
    fx = _handle(s, at, alist, blist, linalg=True)
    assert_path(fx, s, (32, 48), 2)
    n0 = fx.info().n_elyte_charged
    dz = np.zeros(at.nlocal)
    liq = at.echeck[:at.nlocal] == 0
    dz[liq] = np.random.default_rng(61).uniform(-1.0, 1.0, size=int(liq.sum()))
    at.x[:, 2] += dz[at.owner]
    at.q[at.owner == on] = q_on
    at.q[at.owner == off] = 0.0
    q = _update(fx, s, at)
    assert fx.info().n_elyte_charged == n0 and fx.info().zn_cols in (32, 48)
    b_o = check_sk_b(fx, s, at, alist, blist, "charge switched")
    check_charges(fx, s, at, q, b_o, "charge switched")
    fx.close()


def test_the_8192_atom_threshold_and_switching_across_it():
    """exactly 8192 charged electrolyte atoms take the window, 8191 do not; 8192 -> 8191 -> 8192 by switching one charge without
    a re-neighbour flips the path at each list rebuild inside b_cal, with the oracle's b throughout"""
    s = _medium(seed=67)
    sol = np.nonzero(s.echeck == 0)[0]
    s.q[sol[8192:]] = 0.0
    at, alist, blist = neighbor.build_lists(s)
    fx = _handle(s, at, alist, blist)
    assert fx.info().n_elyte_charged == 8192
    fx.b_cal(at)
    assert_path(fx, s, (32, 48), 2)
    check_sk_b(fx, s, at, alist, blist, "8192")
    k = int(sol[4000])
    qk = at.q[k]
    for n_want, q_k, cols in ((8191, 0.0, (0,)), (8192, qk, (32, 48))):
        at.q[at.owner == k] = q_k
        fx.b_cal(at)
        assert fx.info().n_elyte_charged == n_want
        assert_path(fx, s, cols, 2)
        check_sk_b(fx, s, at, alist, blist, f"switched to {n_want}")
    fx.close()
    s.q[sol[8191]] = 0.0                                   # a fresh handle on 8191 atoms
    at, alist, blist = neighbor.build_lists(s)
    fy = _handle(s, at, alist, blist)
    assert fy.info().n_elyte_charged == 8191
    fy.b_cal(at)
    assert_path(fy, s, (0,), 2)
    check_sk_b(fy, s, at, alist, blist, "8191")
    fy.close()


def test_two_compartments_fall_back_to_the_full_kernels():
    """a vapour gap splits the liquid in two: the ordered list starts behind the longest empty run, the range that crosses the other
    one (36 A, ~35 grid cells + 15 taps + margins > 48 columns) is too sparse for any candidate schedule, and the handle takes
    the full kernels (conp_fix.cpp zn_build_items) although it has enough charged atoms -- with the oracle's b"""
    s = _vapour_gap()
    at, alist, blist = neighbor.build_lists(s)
    fx = _handle(s, at, alist, blist)
    assert fx.info().n_elyte_charged >= 8192
    fx.b_cal(at)
    assert_path(fx, s, (0,), 2)
    check_sk_b(fx, s, at, alist, blist, "two compartments")
    fx.close()


# ---- the largest size -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def big_box():
    """BASELINE configs[4] geometry (16384 / 262144): the oracle's S(k) over all k and the k-space b of 64 sampled electrode rows,
    computed once"""
    s = systems.synthetic_fast(n_cells_x=64, n_cells_y=32, lz=1200.0, n_elyte=262144, cutoff=12.0, accuracy_relative=1e-6,
                               g_ewald=0.2554)
    at, alist, blist = neighbor.build_lists(s)
    rows = np.random.default_rng(71).choice(16384, 64, replace=False)
    rows = np.unique(np.concatenate([rows, [0, 8191, 16383]]))
    sr, si, b_o, ks = oracle_sk_and_b(s, at, alist, blist, rows=rows)
    ks.close()
    return s, at, alist, blist, rows, sr, si, b_o


def test_largest_box_structure_factors_and_sampled_b_against_the_oracle(big_box):
    s, at, alist, blist, rows, sr, si, b_o = big_box
    assert len(rows) >= 64
    fx = _handle(s, at, alist, blist)
    fx.b_cal(at)
    assert_path(fx, s, (32, 48), 2)
    sr_g, si_g = fx.sfac()
    b_g = fx.vectors()[0][rows]
    e_s = sk_err(sr_g, si_g, sr, si)
    e_b = np.abs(b_g - b_o).max() / np.abs(b_o).max()
    print(f"262144 atoms: S(k) {e_s:.2e}, b (sampled rows) {e_b:.2e} of max")
    assert e_s < SK_BAR and e_b < B_BAR
    fx.close()


# ---- the bench's timed charges -------------------------------------------------------------------------------------------------
def test_bench_headline_charges_match_the_oracle(tmp_path):
    """bench.py's headline run dumps the charges of its last timed update: electrode charges = S b_oracle + dV S d, electrolyte
    charges unchanged bit for bit"""
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "headline", "--steps", "5",
                        "--warmup", "2", "--dump-outputs", str(tmp_path / "out")], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-2000:]
    q = np.load(tmp_path / "out" / "q.npy")
    s = systems.synthetic_fast()
    at, alist, blist = neighbor.build_lists(s)
    assert q.shape == at.q.shape
    fx = _handle(s, at, alist, blist, linalg=True)
    assert_path(fx, s, (32, 48), 2)
    _, _, b_o, ks = oracle_sk_and_b(s, at, alist, blist)
    ks.close()
    own = np.arange(len(q)) < at.nlocal
    assert np.array_equal(q[own & (at.echeck == 0)], at.q[own & (at.echeck == 0)])
    check_charges(fx, s, at, q, b_o, "bench headline")
    fx.close()


# ---- overflow reporting of the device-resident entries ---------------------------------------------------------------------------
def test_device_overflow_is_reported_by_the_next_post_neighbor():
    """pre_force_device with an atom outside its window, then conp_fix_post_neighbor with no device-resident call between: the
    re-neighbour finishes its list build (window back on at the new positions) and returns CONP_ERR_NUMERIC instead of clearing
    the flag unseen; the next update's charges are the oracle's"""
    import torch
    s = _medium(seed=29)
    at, alist, blist = neighbor.build_lists(s)
    fx = _handle(s, at, alist, blist, linalg=True)
    assert_path(fx, s, (32, 48), 2)
    j = int(np.nonzero((at.echeck[:at.nlocal] == 0) & (at.q[:at.nlocal] != 0))[0][123])
    at.x[at.owner == j, 2] += 60.0
    d_x = torch.from_numpy(np.ascontiguousarray(at.x)).cuda(); d_q = torch.from_numpy(at.q.copy()).cuda()
    fx.pre_force_device(d_x.data_ptr(), d_q.data_ptr(), s.potdiff)
    torch.cuda.synchronize()
    with pytest.raises(capi.ConpError) as e:
        fx.post_neighbor(at)
    assert e.value.code == -4 and "z-window" in e.value.msg
    assert_path(fx, s, (32, 48), 2)                     # the list was built at the new positions
    fx.pre_force_device(d_x.data_ptr(), d_q.data_ptr(), s.potdiff)
    torch.cuda.synchronize()
    q = d_q.cpu().numpy()
    fx.pre_force_device(d_x.data_ptr(), d_q.data_ptr(), s.potdiff)     # no error: that update stayed inside its windows
    torch.cuda.synchronize()
    fx.b_cal(at)
    b_o = check_sk_b(fx, s, at, alist, blist, "device overflow, post_neighbor")
    check_charges(fx, s, at, q, b_o, "device overflow, post_neighbor")
    fx.close()


def test_graph_replay_reports_a_window_overflow_on_the_next_call():
    """CONP_GRAPH=1: the update is replayed as a captured graph from its second call on.  An atom leaving its window after the
    capture raises the flag in a replay; the next call returns CONP_ERR_NUMERIC as the direct path does, the handle runs without
    the window from then on, and its charges are the oracle's"""
    import torch
    s = _medium(seed=73)
    at, alist, blist = neighbor.build_lists(s)
    os.environ["CONP_GRAPH"] = "1"                       # read when the handle is created
    try:
        fx = FixConp(s)
    finally:
        del os.environ["CONP_GRAPH"]
    fx.init_lists(alist, blist); fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)                 # (electrode charges only: b does not see them)
    assert_path(fx, s, (32, 48), 2)
    d_x = torch.from_numpy(np.ascontiguousarray(at.x)).cuda(); d_q = torch.from_numpy(at.q.copy()).cuda()
    for _ in range(3):                                   # direct, captured, replayed
        fx.pre_force_device(d_x.data_ptr(), d_q.data_ptr(), s.potdiff)
        torch.cuda.synchronize()
    j = int(np.nonzero((at.echeck[:at.nlocal] == 0) & (at.q[:at.nlocal] != 0))[0][321])
    at.x[at.owner == j, 2] += 60.0
    d_x.copy_(torch.from_numpy(np.ascontiguousarray(at.x)))
    fx.pre_force_device(d_x.data_ptr(), d_q.data_ptr(), s.potdiff)        # replayed: the flag is raised on the device
    torch.cuda.synchronize()
    with pytest.raises(capi.ConpError) as e:
        fx.pre_force_device(d_x.data_ptr(), d_q.data_ptr(), s.potdiff)
    assert e.value.code == -4 and "z-window" in e.value.msg
    assert fx.info().zn_cols == 0
    for _ in range(3):                                   # direct, captured, replayed: all on the full kernels
        fx.pre_force_device(d_x.data_ptr(), d_q.data_ptr(), s.potdiff)
        torch.cuda.synchronize()
    q = d_q.cpu().numpy()
    fx.b_cal(at)
    assert fx.info().zn_cols == 0
    b_o = check_sk_b(fx, s, at, alist, blist, "graph replay overflow")
    check_charges(fx, s, at, q, b_o, "graph replay overflow")
    fx.close()
