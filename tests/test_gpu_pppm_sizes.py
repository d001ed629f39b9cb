"""-m gpu: the PPPM mesh path (`pppm` keyword) at production mesh sizes, every stencil order and the edges of the box, against the
CPU oracle's PPPM chain (oracle_py.Pppm: b_cal, make_rho, group_potential) on identical inputs, and against the Ewald b.

conp_pppm.hip picks its kernels by size; tests/test_gpu_pppm.py runs the reference decks, which all take the same choice.  `select`
below restates that choice (DESIGN.md section 8 holds the same table) as arithmetic on (nx, ny, nz, order, nl), and every case
asserts the path it is meant for BEFORE it compares numbers: a later change of a threshold fails the case instead of turning it
back into a deck-sized test.

The reference side: the oracle's transform is a plain O(N n) DFT per axis -- minutes on the 2.5 M and 7.5 M point meshes here -- so
the large cases solve the oracle's own density brick with the oracle's own influence function through numpy.fft (Pppm(fast=True));
tests/test_oracle_pin.py pins that step to the plain DFT at 1e-13 (measured distance of the two, relative to the largest mesh
value: 8e-16 and 6e-16 on the pinned meshes, 4.0e-15 on 72 x 64 x 540, where one plain-DFT solve takes 20.5 s and the FFT one 0.29 s).
An FFT's rounding error grows with log n, the plain DFT's with n, so the reference is not the weaker side on the long lines and every
case holds the project's tolerances unwidened: 1e-11 for b, 1e-12 for the density bricks, 1e-10 for the potentials, all relative to
the largest entry of the reference vector (helpers.rel_err).  Measured on the MI355X: b 0.9e-15 .. 7e-15, bricks <= 6e-16,
potentials <= 2e-15 in every case.

The Ewald leg: EWALD_ORACLE holds PPPM-vs-Ewald of the ORACLE's b, measured on the CPU; the library is asserted against twice that
(the factor covers the choice of a round number only: oracle and library agree to 1e-11, the mesh error is the same).  Orders
below 4 have no Ewald leg (their mesh accuracy is not known in advance); the oracle leg stays.

Reference-side times (one CPU core): oracle b_cal 0.8 s (headline ffield) and 2.1 s (headline slab), the Ewald b of the headline box
(99773 k vectors, 4096 rows) 4.4 s and 13.5 s; the whole module takes 17 s."""
import numpy as np
import pytest

import oracle_py
from conp_amd import ConpError, FixConp, capi, neighbor, systems
from helpers import push_outside, rel_err

pytestmark = pytest.mark.gpu

# ---- the kernel selection of conp_pppm.hip as plain arithmetic ---------------------------------------------------------------
PLANE_LDS_MAX = 128 * 1024       # pppm_fft_xy_kernel: a z-plane (two complex buffers + twiddles of x and y) has to fit
LINE_LDS_MAX = 160 * 1024        # a workgroup's LDS: longer lines are refused at setup
IN_PASS_MAX_ATOMS, IN_PASS_MAX_NZ, IN_PASS_MAX_ORDER2 = 8192, 1024, 64
MAX_SLAB_PARTS = 1024


def radices(n):
    """fft_factor: 4s first, then 2, 3, 5; None when n is not 2,3,5-smooth"""
    out = []
    while n % 4 == 0:
        out.append(4); n //= 4
    for r in (2, 3, 5):
        while n % r == 0:
            out.append(r); n //= r
    return out if n == 1 else None


def plane_lds(nx, ny):
    return 2 * nx * ny * 16 + 16 * (nx + ny)


def line_lds(n):
    """(lines per workgroup, dynamic LDS) of one axis' transform: pppm_fft_kernel for smooth n, pppm_dft_kernel otherwise"""
    if radices(n):
        xs = 0
        while xs < 4 and n * 32 * (2 << xs) <= 64 * 1024:
            xs += 1
        return 1 << xs, 2 * n * (1 << xs) * 16 + 16 * n
    xt = min(max(48 * 1024 // (n * 16), 1), 16)
    return xt, (2 * n * xt + 2 * n) * 8


def select(mesh, order, nl, forced_spread_launch=False):
    """which kernels launch_pppm_b / launch_pppm_poisson run for this mesh, order and number of charged electrolyte atoms"""
    nx, ny, nz = mesh
    all_smooth = all(radices(n) for n in mesh)
    planes = all_smooth and plane_lds(nx, ny) <= PLANE_LDS_MAX                 # x and y of a z-plane in one workgroup
    axes = tuple("plane" if planes and c < 2 else ("fft" if radices(n) else "dft") for c, n in enumerate(mesh))
    in_pass = (planes and not forced_spread_launch and nl <= IN_PASS_MAX_ATOMS and nz <= IN_PASS_MAX_NZ
               and order * order <= IN_PASS_MAX_ORDER2)
    tpa = min(order ** 3, 256)                                                # threads per atom of pppm_spread_kernel
    groups = max(-(-nl // (256 // tpa)), 1)
    npass = -(-groups // MAX_SLAB_PARTS)
    return dict(axes=axes, spread="in_pass" if in_pass else "launch", rho_in_im=planes and not in_pass, npass=npass,
                slab_parts=nz if in_pass else -(-groups // npass), rounds=-(-order ** 3 // 256), lines_z=line_lds(nz)[0])


# PPPM-vs-Ewald of the oracle's b (rel_err), measured on the CPU with the inputs of the case
EWALD_ORACLE = {
    "dilute_slab_tall": 6.1036e-05,
    "dilute_27x24x154": 1.9163e-05,
    "dilute_27x22x144": 1.9350e-05,
    "dilute_28x24x144": 1.9356e-05,
    "dilute_order6": 1.9231e-05,
    "dilute_order7": 1.9273e-05,
    "dilute_order8": 1.9280e-05,
    "boundary_80": 8.5303e-08,
    "boundary_81": 8.5214e-08,
    "medium_ffield": 7.5040e-08,
    "headline_ffield": 8.6131e-08,
    "headline_slab": 1.4214e-07,
}


# ---- drivers ------------------------------------------------------------------------------------------------------------------
def _handle(s, mesh, order, forced_spread_launch=False):
    at, alist, blist = neighbor.build_lists(s)
    if forced_spread_launch:
        capi.load_library().conp_debug_set_paths(capi.PATH_PPPM_SPREAD_LAUNCH)      # (the conftest fixture switches it off again)
    fx = FixConp(s, extra_args=["pppm"], pppm_mesh=mesh, pppm_order=order)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    return at, fx


def _nl(at):
    n = at.nlocal
    return int(np.count_nonzero((at.echeck[:n] == 0) & (at.q[:n] != 0)))


def _xele(fx, at):
    loc = {int(t): i for i, t in enumerate(at.tag[:at.nlocal])}
    return np.array([at.x[loc[int(t)]] for t in fx.maps()["eleall2tag"]])


def _ewald_b(oracle, s, at, xele):
    ks = oracle_py.KSpace.from_system(oracle, s)
    sr, si = ks.sincos_b(at.x, at.q, at.echeck, at.nlocal)
    csk, snk = ks.ele_trig(xele)
    b = ks.bbb(csk, snk, sr, si)
    if s.slabflag:
        oracle.orc_slabcorr(ks.h, at.nlocal, np.ascontiguousarray(at.x), at.q, at.echeck, len(xele), np.ascontiguousarray(xele), b)
    ks.close()
    return b


def _check_b(oracle, s, at, fx, pp, key=None, label=""):
    """km_b_cal (k-space part + slab term, every electrode row) against the oracle, and against Ewald when the case has a figure"""
    xele = _xele(fx, at)
    got = fx.km_b_cal(at)
    want = pp.b_cal(at.x, at.q, at.echeck, at.nlocal, xele)
    assert np.abs(want).max() > 0
    e = rel_err(got, want)
    print(f"[{label or key}] b vs oracle {e:.3e} over {len(want)} rows")
    assert e < 1e-11
    if key is not None:
        b_ew = _ewald_b(oracle, s, at, xele)
        e_o, e_l = rel_err(want, b_ew), rel_err(got, b_ew)
        print(f"[{key}] PPPM vs Ewald: oracle {e_o:.4e} (recorded {EWALD_ORACLE[key]:.4e}), library {e_l:.4e}")
        assert e_o == pytest.approx(EWALD_ORACLE[key], rel=0.01)              # the recorded figure belongs to these inputs
        assert e_l < 2 * EWALD_ORACLE[key]
    return got, want


def _charge_electrodes(at, seed=11):
    """electrode charges for the bricks and potentials (a solve is not what is under test): seeded, opposite sign on the two
    electrodes, ghosts like their owners"""
    n = at.nlocal
    ele = at.echeck[:n] != 0
    at.q[:n][ele] = np.random.default_rng(seed).uniform(0.005, 0.02, int(ele.sum())) * at.echeck[:n][ele]
    at.q[n:] = at.q[at.owner[n:]]


def _check_bricks(s, at, fx, pp, mesh, label):
    """pppm_make_rho: electrode brick, electrolyte brick and their sum at every mesh point; brick total times cell volume = charge"""
    n = at.nlocal
    d, e, l = fx.pppm_make_rho(at, mesh[0] * mesh[1] * mesh[2])
    d_o, e_o, l_o = pp.make_rho(mesh, at.x, at.q, at.echeck, n)
    assert np.abs(e_o).max() > 0 and np.abs(l_o).max() > 0 and np.abs(d_o).max() > 0
    errs = rel_err(e, e_o), rel_err(l, l_o), rel_err(d, d_o)
    print(f"[{label}] bricks vs oracle (electrode, electrolyte, sum) " + " ".join(f"{v:.3e}" for v in errs))
    assert max(errs) < 1e-12
    dv = (s.prd[0] / mesh[0]) * (s.prd[1] / mesh[1]) * (s.prd[2] * s.slab_volfactor / mesh[2])
    ele = at.echeck[:n] != 0
    # 1e-10 is the bound of the deck-sized brick test (1280 atoms); the rounding of the weights and of the total grows with the
    # number of atoms spread, so the bound is scaled by it on the boxes that hold more
    tol = 1e-10 * max(1.0, np.count_nonzero(at.q[:n]) / 1280.0)
    assert e.sum() * dv == pytest.approx(at.q[:n][ele].sum(), abs=tol)
    assert l.sum() * dv == pytest.approx(at.q[:n][~ele].sum(), abs=tol)


def _check_potentials(at, fx, pp, frac, label, extra=()):
    """pppm_group_potential on a seeded sample of the atoms plus some electrode atoms (and `extra`)"""
    n = at.nlocal
    sel = (np.random.default_rng(4).random(n) < frac).astype(np.int32)
    sel[np.nonzero(at.echeck[:n] != 0)[0][:64]] = 1
    sel[list(extra)] = 1
    got = fx.pppm_group_potential(at, sel)
    want = pp.group_potential(at.x, at.q, at.echeck, n, sel)
    pick = sel != 0
    assert np.abs(want[pick]).max() > 0
    e = rel_err(got[pick], want[pick])
    print(f"[{label}] potentials vs oracle {e:.3e} over {int(pick.sum())} atoms")
    assert e < 1e-10
    return int(pick.sum())


def _move_electrolyte(at, rng, amp=0.3):
    """random displacements of the electrolyte (no re-neighbouring needed), the ghosts with their owners"""
    n = at.nlocal
    d = rng.uniform(-amp, amp, (n, 3)) * (at.echeck[:n] == 0)[:, None]
    at.x[:n] += d
    at.x[n:] += d[at.owner[n:]]


# ---- 1, 2: the headline box ---------------------------------------------------------------------------------------------------
def test_headline_box_per_axis_x_and_y_and_sixteen_spreading_passes(oracle):
    """4096 electrode / 32768 electrolyte atoms, 72 x 64 x 540, order 5: the plane (149632 bytes) does not fit in LDS, so x and y go
    through pppm_fft_kernel's axis 0 / axis 1 addressing (real input on axis 0, influence function on the way out of the forward z
    pass, real part only out of the backward z pass); radices 4, 2, 3, 5 all occur; pppm_spread_kernel + zero_kernel with 16
    atom groups per workgroup.  b, the three bricks and the potentials of 2 % of the atoms."""
    s = systems.synthetic_fast()
    mesh, order = (72, 64, 540), 5
    at, fx = _handle(s, mesh, order)
    sel = select(mesh, order, _nl(at))
    assert _nl(at) == 32768 and plane_lds(72, 64) == 149632 > PLANE_LDS_MAX
    assert sel["axes"] == ("fft", "fft", "fft") and sel["spread"] == "launch" and not sel["rho_in_im"]
    assert sel["npass"] == 16 and sel["slab_parts"] == 1024 and sel["lines_z"] == 2
    assert {r for n in mesh for r in radices(n)} == {2, 3, 4, 5}
    pp = oracle_py.Pppm(oracle, s, mesh, order, fast=True)
    _check_b(oracle, s, at, fx, pp, key="headline_ffield")
    _charge_electrodes(at)
    _check_bricks(s, at, fx, pp, mesh, "headline_ffield")
    assert _check_potentials(at, fx, pp, 0.02, "headline_ffield") >= 500
    _check_b(oracle, s, at, fx, pp, label="headline_ffield, after the bricks and potentials")
    pp.close(); fx.close()


def test_headline_box_slab_with_a_z_line_of_1620_points(oracle):
    """slab geometry, 72 x 64 x 1620: nz > 1024, a z line (1620 = 4 3^4 5) is transformed alone by its workgroup (77760 bytes of
    LDS); the slab sum of 32768 atoms comes in 1024 partial sums.  b only."""
    s = systems.synthetic_fast(mode="slab")
    mesh, order = (72, 64, 1620), 5
    at, fx = _handle(s, mesh, order)
    sel = select(mesh, order, _nl(at))
    assert sel["axes"] == ("fft", "fft", "fft") and sel["spread"] == "launch" and sel["npass"] == 16 and sel["slab_parts"] == 1024
    assert line_lds(1620) == (1, 77760) and radices(1620) == [4, 3, 3, 3, 3, 5]
    pp = oracle_py.Pppm(oracle, s, mesh, order, fast=True)
    got, want = _check_b(oracle, s, at, fx, pp, key="headline_slab")
    # the slab term alone is far above the tolerance: the same chain without it
    s0 = s.copy(); s0.slabflag = 0
    pp0 = oracle_py.Pppm(oracle, s0, mesh, order, fast=True)
    b0 = pp0.b_cal(at.x, at.q, at.echeck, at.nlocal, _xele(fx, at))
    assert rel_err(b0, want) > 1e3 * 1e-11
    pp0.close(); pp.close(); fx.close()


# ---- 3: the density brick in `im`, update after update -------------------------------------------------------------------------
def test_consecutive_updates_reuse_the_clean_im_brick(oracle):
    """12288 electrolyte atoms (> 8192) on 40 x 36 x 270: the plane fits, so pppm_spread_kernel spreads into `im` and the last backward
    pass leaves `im` zero for the NEXT update, which skips the clearing launch.  Three updates with the electrolyte moved in
    between, then the bricks and the potentials (they use re / im too) with further updates behind them: each against the oracle at
    the positions of the moment."""
    s = systems.synthetic_fast(n_cells_x=16, n_cells_y=8, lz=300.0, n_elyte=12288)
    mesh, order = (40, 36, 270), 5
    at, fx = _handle(s, mesh, order)
    nl = _nl(at)
    sel = select(mesh, order, nl)
    assert nl == 12288 > IN_PASS_MAX_ATOMS and plane_lds(40, 36) <= PLANE_LDS_MAX
    assert sel["axes"] == ("plane", "plane", "fft") and sel["spread"] == "launch" and sel["rho_in_im"] and sel["npass"] == 6
    pp = oracle_py.Pppm(oracle, s, mesh, order, fast=True)
    rng = np.random.default_rng(21)
    _check_b(oracle, s, at, fx, pp, key="medium_ffield")
    seen = []
    for u in (2, 3):
        _move_electrolyte(at, rng)
        got, _ = _check_b(oracle, s, at, fx, pp, label=f"medium_ffield, update {u}")
        seen.append(got)
    assert rel_err(seen[1], seen[0]) > 1e3 * 1e-11                  # the moves are far above the tolerance: a stale brick would show
    _charge_electrodes(at)
    _check_bricks(s, at, fx, pp, mesh, "medium_ffield")
    _move_electrolyte(at, rng)
    _check_b(oracle, s, at, fx, pp, label="medium_ffield, update behind make_rho")
    _check_potentials(at, fx, pp, 0.05, "medium_ffield")
    _move_electrolyte(at, rng)
    _check_b(oracle, s, at, fx, pp, label="medium_ffield, update behind the potentials")
    _check_b(oracle, s, at, fx, pp, label="medium_ffield, the same again")
    pp.close(); fx.close()


# ---- 4: few atoms, tall mesh ---------------------------------------------------------------------------------------------------
def test_tall_mesh_switches_a_deck_to_the_spreading_launch(oracle):
    """dilute deck, slab, 27 x 24 x 1080: few atoms, but nz > 1024, so the default is the spreading launch (into `im`) and a z line per
    workgroup; two updates"""
    s = systems.deck("dilute", "slab", etypes=True)
    mesh, order = (27, 24, 1080), 5
    at, fx = _handle(s, mesh, order)
    sel = select(mesh, order, _nl(at))
    assert _nl(at) <= IN_PASS_MAX_ATOMS and mesh[2] > IN_PASS_MAX_NZ
    assert sel["axes"] == ("plane", "plane", "fft") and sel["spread"] == "launch" and sel["rho_in_im"] and sel["npass"] == 1
    assert sel["lines_z"] == 1
    pp = oracle_py.Pppm(oracle, s, mesh, order, fast=True)
    _check_b(oracle, s, at, fx, pp, key="dilute_slab_tall")
    _move_electrolyte(at, np.random.default_rng(5))
    _check_b(oracle, s, at, fx, pp, label="dilute_slab_tall, update 2")
    pp.close(); fx.close()


# ---- 5: the largest plane that fits in LDS and the first that does not ---------------------------------------------------------
def test_lds_boundary_of_the_plane_kernel(oracle):
    """80 x 50 is the largest plane pppm_fft_xy_kernel takes (130080 bytes of dynamic LDS, the charges spread inside the pass), 81 x 50
    (131696) the first that goes per axis.  Both against the oracle; the two b vectors agree within the sum of their mesh errors."""
    s = systems.synthetic_fast(n_cells_x=16, n_cells_y=8, lz=120.0, n_elyte=4096)
    order, b = 5, {}
    for key, mesh in (("boundary_80", (80, 50, 120)), ("boundary_81", (81, 50, 120))):
        at, fx = _handle(s, mesh, order)
        sel = select(mesh, order, _nl(at))
        assert _nl(at) == 4096 <= IN_PASS_MAX_ATOMS
        if mesh[0] == 80:
            assert plane_lds(80, 50) == 130080 <= PLANE_LDS_MAX and plane_lds(80, 51) > PLANE_LDS_MAX
            assert sel["axes"] == ("plane", "plane", "fft") and sel["spread"] == "in_pass"
        else:
            assert plane_lds(81, 50) == 131696 > PLANE_LDS_MAX
            assert sel["axes"] == ("fft", "fft", "fft") and sel["spread"] == "launch" and not sel["rho_in_im"]
        pp = oracle_py.Pppm(oracle, s, mesh, order, fast=True)
        b[key], _ = _check_b(oracle, s, at, fx, pp, key=key)
        _charge_electrodes(at)
        _check_bricks(s, at, fx, pp, mesh, key)
        _check_potentials(at, fx, pp, 0.1, key)
        pp.close(); fx.close()
    assert rel_err(b["boundary_81"], b["boundary_80"]) < 2 * (EWALD_ORACLE["boundary_80"] + EWALD_ORACLE["boundary_81"])


# ---- 6: axes that are not 2,3,5-smooth ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mesh,axes", [((27, 24, 154), ("fft", "fft", "dft")),       # 154 = 2 7 11: plain DFT along z only
                                       ((27, 22, 144), ("fft", "dft", "fft")),       # one planar axis each
                                       ((28, 24, 144), ("dft", "fft", "fft"))])
def test_one_axis_not_smooth(oracle, mesh, axes):
    """a mesh with one length that is not 2,3,5-smooth: that axis takes pppm_dft_kernel, the other two pppm_fft_kernel (plain flags,
    the influence function in a launch of its own), the charges the spreading launch"""
    s = systems.deck("dilute", "ffield", etypes=True)
    at, fx = _handle(s, mesh, 5)
    sel = select(mesh, 5, _nl(at))
    assert sel["axes"] == axes and sel["spread"] == "launch" and not sel["rho_in_im"]
    pp = oracle_py.Pppm(oracle, s, mesh, 5)
    _check_b(oracle, s, at, fx, pp, key="dilute_%dx%dx%d" % mesh)
    _charge_electrodes(at)
    _check_potentials(at, fx, pp, 0.3, "dilute_%dx%dx%d" % mesh)
    pp.close(); fx.close()


# ---- 7: stencil orders ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order,forced", [(1, False), (2, False), (3, False), (6, False), (7, False), (8, False), (7, True), (8, True)])
def test_stencil_orders(oracle, order, forced):
    """orders 1, 2 (nlower = 0), 3, 6, 7 and 8 (the library's and the oracle's maximum, one above LAMMPS': w[3][8] and coeff[64]
    filled exactly) on the dilute deck: b inside the forward pass; for 7 and 8 also through the spreading launch, whose 343 / 512
    stencil points take two rounds of 256 threads.  The bricks and the potentials always use that kernel."""
    s = systems.deck("dilute", "ffield", etypes=True)
    mesh = (27, 24, 144)
    at, fx = _handle(s, mesh, order, forced_spread_launch=forced)
    sel = select(mesh, order, _nl(at), forced)
    assert sel["spread"] == ("launch" if forced else "in_pass") and sel["rounds"] == (2 if order >= 7 else 1)
    assert (-((order - 1) // 2) == 0) == (order <= 2)                 # nlower
    pp = oracle_py.Pppm(oracle, s, mesh, order)
    _check_b(oracle, s, at, fx, pp, key=f"dilute_order{order}" if order >= 4 else None, label=f"dilute_order{order}")
    _charge_electrodes(at)
    _check_bricks(s, at, fx, pp, mesh, f"dilute_order{order}")
    _check_potentials(at, fx, pp, 0.3, f"dilute_order{order}")
    pp.close(); fx.close()


def test_order_out_of_range_and_missing_order_are_errors():
    """order 9: a negative status with the plan's message; order 0: the reference's missing-kspace-style error (fix_conp.cpp:404).
    Both are raised by linalg_init before anything is launched."""
    s = systems.deck("dilute", "ffield", etypes=True)
    at, alist, blist = neighbor.build_lists(s)
    for order, text in ((9, "pppm order out of range"), (0, "couldn't detect a pppm/conp kspace style")):
        fx = FixConp(s, extra_args=["pppm"], pppm_mesh=(27, 24, 144), pppm_order=order)
        fx.init_lists(alist, blist)
        with pytest.raises(ConpError) as e:
            fx.setup_post_neighbor(at)
        assert e.value.code < 0 and text in str(e.value)
        fx.close()


@pytest.mark.parametrize("nz", [3456, 4096, 5121])
def test_mesh_line_that_cannot_fit_in_lds_is_refused_at_setup(nz):
    """a mesh line is transformed in LDS: 48 n bytes for a smooth length above 1024 (3456 = 2^7 3^3: 165888), 32 n for any other
    (5121 = 3^2 569: 163872) against the 163840 a workgroup has.  Such a launch could not run; the mesh is CONP_ERR_ARG at setup."""
    assert line_lds(nz)[1] > LINE_LDS_MAX and line_lds(3375)[1] <= LINE_LDS_MAX and line_lds(5110)[1] <= LINE_LDS_MAX
    s = systems.deck("dilute", "ffield", etypes=True)
    at, alist, blist = neighbor.build_lists(s)
    fx = FixConp(s, extra_args=["pppm"], pppm_mesh=(27, 24, nz), pppm_order=5)
    fx.init_lists(alist, blist)
    with pytest.raises(ConpError) as e:
        fx.setup_post_neighbor(at)
    assert e.value.code == -1 and "does not fit in the LDS" in str(e.value)
    fx.close()


# ---- 8: atoms outside the periodic box ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forced", [False, True])
def test_atoms_outside_the_box_and_on_its_upper_face(oracle, forced):
    """between re-neighbourings LAMMPS leaves atoms up to a fraction of the skin outside the box: a dozen electrolyte atoms up to 1 A
    outside in x, y and z, unwrapped, and one exactly on boxhi in each direction (mesh index n, wrapped by the stencil); ghosts moved
    with their owners.  tests/test_oracle_pin.py checks the oracle's own handling of these positions on the CPU."""
    s = systems.deck("dilute", "ffield", etypes=True)
    mesh, order = (27, 24, 144), 5
    at, fx = _handle(s, mesh, order, forced_spread_launch=forced)
    moved = push_outside(s, at)
    n = at.nlocal
    assert len(moved) == 15 and (np.any(at.x[:n] > s.boxhi, axis=1) | np.any(at.x[:n] < s.boxlo, axis=1)).sum() == 12
    assert all(np.any(at.x[i] == s.boxhi) for i in moved[12:])
    assert select(mesh, order, _nl(at), forced)["spread"] == ("launch" if forced else "in_pass")
    pp = oracle_py.Pppm(oracle, s, mesh, order)
    _check_b(oracle, s, at, fx, pp, label="dilute_outside")
    _charge_electrodes(at)
    _check_bricks(s, at, fx, pp, mesh, "dilute_outside")
    _check_potentials(at, fx, pp, 0.3, "dilute_outside", extra=moved)
    pp.close(); fx.close()
