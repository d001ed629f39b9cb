"""-m gpu: conp_ewald_compute_forces_device / conp_pppm_compute_forces_device -- the reciprocal-space forces, energy, virial and
per-atom energies from DEVICE arrays, enqueued on the handle's stream without a host round trip.

(1) Ewald against the numpy definitions of tests/ewald_force_ref.py, zero-charge probes included;  (2) several blocks and a ragged
    last one (conp_debug_set_ew_block);  (3) accumulation into d_f and ordering: three calls, one synchronisation;  (4) NULL
    outputs;  (5) a whole step on the device: the update, then the forces, nothing between them;  (6) PPPM against the numpy mesh
    reference of tests/pppm_force_ref.py, one spread per call, a kept electrolyte brick is not used;  (7) refusals, and the host
    entries after a device entry;  (8) guard zones.
Bounds (those of tests/test_gpu_ewald_forces.py and tests/test_gpu_pppm_forces.py): forces 1e-10 max|f|; energy, virial and per-atom
energies 1e-11 of the unsubtracted scale (qs sum ug |S|^2, or qs (V / 2) sum G |rho^|^2 / N^2).
Measured on an MI355X (fractions of the bound): see DESIGN.md section 14."""
import functools
import os
import subprocess
import sys
from types import SimpleNamespace

import numpy as np
import pytest

import ewald_force_ref as eref
import pppm_force_ref as pref
from conp_amd import ConpError, capi
from test_gpu_ewald_potential import _add_probes, _handle as _ewald_handle, _system
from test_gpu_pppm_forces import _handle as _pppm_handle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MESH0 = pref.ROWS[0]          # ("dilute", "ffield", (27, 24, 144), 5)


def _compare(tag, got, want, bound):
    err = float(np.abs(np.asarray(got) - np.asarray(want)).max())
    print(f"{tag}: max error {err:.3e}, bound {bound:.3e} ({err / bound:.3g} of it)")
    assert err <= bound, (tag, err, bound)


def _to_device(at):
    """(d_x, d_q) of all atoms of `at`, owned first, as torch tensors; the copies have landed when this returns"""
    import torch
    d_x = torch.from_numpy(np.ascontiguousarray(at.x, dtype=np.float64)).cuda()
    d_q = torch.from_numpy(np.ascontiguousarray(at.q, dtype=np.float64)).cuda()
    torch.cuda.synchronize()
    return d_x, d_q


def _call(entry, d_x, d_q, n, f=True, ev=True, eatom=True, pre=None, times=1):
    """`times` calls of a device entry with fresh output tensors and NO synchronisation between them, one afterwards -> (f, ev, e)
    as numpy arrays (None where the output was NULL).  Outputs that are overwritten start as NaN."""
    import torch
    d_f = d_ev = d_e = None
    if f:
        d_f = torch.zeros((n, 3), dtype=torch.float64, device="cuda") if pre is None else torch.from_numpy(pre.copy()).cuda()
    if ev:
        d_ev = torch.full((7,), float("nan"), dtype=torch.float64, device="cuda")
    if eatom:
        d_e = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    for _ in range(times):
        entry(d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr() if f else 0, d_ev.data_ptr() if ev else 0, d_e.data_ptr() if eatom else 0)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (d_f, d_ev, d_e))


def _check(tag, got, want, probes=()):
    """f, ev, eatom of a device entry against a reference (f, E, W, e, scale); the probes' entries are exact zeros"""
    (gf, gev, ge), (f, E, W, e, scale) = got, want
    if len(probes):
        assert np.all(gf[probes] == 0.0) and np.all(ge[probes] == 0.0)
    assert np.abs(f).max() > 0 and scale > 0
    _compare(f"{tag} force", gf, f, 1e-10 * np.abs(f).max())
    _compare(f"{tag} energy", gev[0], E, 1e-11 * scale)
    _compare(f"{tag} virial", gev[1:], W, 1e-11 * scale)
    _compare(f"{tag} eatom", ge, e, 1e-11 * scale)


def _ewald_reference(fx, s, x, q):
    T = eref.handle_tables(fx, s)
    n = len(q)
    S = eref.structure_factor(x, q, T["kv"])
    E, W = eref.energy_virial(S, x, q, T["kv"], T["ug"], T["g"], T["V"], T["qs"], T["slab"], T["L"])
    f, e = eref.forces_eatom(S, x, q, T["kv"], T["ug"], T["g"], T["V"], T["qs"], np.arange(n), T["slab"], T["L"])
    return f, E, W, e, T["qs"] * eref.ksum(S, T["ug"])


@functools.lru_cache(maxsize=None)
def ewald_case(name, mode):
    """an Ewald handle after an update, zero-charge probes added, its atoms on the device and the numpy reference at them: formed
    once per process, shared by the tests (the device entries keep no state between calls)"""
    s = _system(name, mode)
    at, alist, blist, fx = _ewald_handle(s)
    n = at.nlocal
    probes = _add_probes(s, at)
    x, q = np.ascontiguousarray(at.x[:n]), np.ascontiguousarray(at.q[:n])
    d_x, d_q = _to_device(at)
    return SimpleNamespace(s=s, at=at, alist=alist, blist=blist, fx=fx, n=n, probes=probes, d_x=d_x, d_q=d_q,
                           want=_ewald_reference(fx, s, x, q), tag=f"{name}/{mode}")


def _pppm_reference(oracle, s, at, mesh, order):
    f, E, W, e, scale, T = pref.reference(oracle, s, at, mesh, order)
    return f, E, W, e, scale


@functools.lru_cache(maxsize=None)
def pppm_case(row):
    import oracle_py
    deck, mode, mesh, order = row
    s, at, alist, blist, fx = _pppm_handle(deck, mode, mesh, order)
    n = at.nlocal
    probes = _add_probes(s, at)
    d_x, d_q = _to_device(at)
    return SimpleNamespace(s=s, at=at, alist=alist, blist=blist, fx=fx, n=n, probes=probes, d_x=d_x, d_q=d_q, mesh=mesh, order=order,
                           want=_pppm_reference(oracle_py.load(), s, at, mesh, order), tag=f"{deck}/{mode} {mesh} order {order}")


# ---- (1) Ewald against the definitions -------------------------------------------------------------------------------------
def run_ewald_definitions(name, mode):
    c = ewald_case(name, mode)
    _check(c.tag, _call(c.fx.ewald_forces_device, c.d_x, c.d_q, c.n), c.want, c.probes)


@pytest.mark.parametrize("name,mode", [("small", "slab"), ("small", "ffield"), ("dilute", "ffield")])
def test_ewald_matches_the_definitions(name, mode):
    run_ewald_definitions(name, mode)


# ---- (2) several blocks, a ragged last one ---------------------------------------------------------------------------------
def run_ewald_blocks():
    c = ewald_case("dilute", "ffield")
    assert c.n > 2 * 64 and c.n % 64 != 0, c.n        # at least three blocks, the last one ragged
    capi.set_ew_block(64)
    try:
        got = _call(c.fx.ewald_forces_device, c.d_x, c.d_q, c.n)
    finally:
        capi.set_ew_block(0)
    _check(f"{c.tag}, blocks of 64 ({c.n} atoms)", got, c.want, c.probes)


def test_ewald_in_blocks_with_a_ragged_last_block():
    run_ewald_blocks()


# ---- (3) accumulation and ordering -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("provider", ["ewald", "pppm"])
def test_forces_accumulate_outputs_are_overwritten_and_calls_need_no_synchronisation(provider):
    c = ewald_case("dilute", "ffield") if provider == "ewald" else pppm_case(MESH0)
    entry = c.fx.ewald_forces_device if provider == "ewald" else c.fx.pppm_forces_device
    scale, fmax = c.want[4], np.abs(c.want[0]).max()
    f1, ev1, e1 = _call(entry, c.d_x, c.d_q, c.n)
    pre = np.random.default_rng(2).normal(size=(c.n, 3))
    f3, ev3, e3 = _call(entry, c.d_x, c.d_q, c.n, pre=pre, times=3)
    _compare(f"{provider}: pre-fill + 3 calls", f3, pre + 3 * f1, 1e-10 * fmax)
    _compare(f"{provider}: energy and virial of one call", ev3, ev1, 1e-11 * scale)
    _compare(f"{provider}: eatom of one call", e3, e1, 1e-11 * scale)


# ---- (4) NULL outputs ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("provider", ["ewald", "pppm"])
def test_null_outputs(provider):
    c = ewald_case("dilute", "ffield") if provider == "ewald" else pppm_case(MESH0)
    entry = c.fx.ewald_forces_device if provider == "ewald" else c.fx.pppm_forces_device
    scale, fmax = c.want[4], np.abs(c.want[0]).max()
    full = _call(entry, c.d_x, c.d_q, c.n)
    for k, name in enumerate(("d_f", "d_ev", "d_eatom")):
        on = [True, True, True]
        on[k] = False
        got = _call(entry, c.d_x, c.d_q, c.n, f=on[0], ev=on[1], eatom=on[2])
        assert got[k] is None
        if on[0]:
            _compare(f"{provider}, {name} NULL: force", got[0], full[0], 1e-10 * fmax)
        if on[1]:
            _compare(f"{provider}, {name} NULL: energy and virial", got[1], full[1], 1e-11 * scale)
        if on[2]:
            _compare(f"{provider}, {name} NULL: eatom", got[2], full[2], 1e-11 * scale)
    n0 = c.fx.info().pppm_elyte_spreads
    entry(c.d_x.data_ptr(), c.d_q.data_ptr(), 0, 0, 0)          # all three NULL: CONP_OK (anything else raises), nothing done
    assert c.fx.info().pppm_elyte_spreads == n0


# ---- (5) a whole step on the device ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("provider", ["ewald", "pppm"])
def test_a_whole_step_on_the_device(provider, oracle):
    """pre_force_device writes the electrode charges into d_q; the force entry behind it on the same stream reads them"""
    import torch
    if provider == "ewald":
        s = _system("dilute", "ffield")
        at, alist, blist, fx = _ewald_handle(s)
        entry = fx.ewald_forces_device
    else:
        deck, mode, mesh, order = MESH0
        s, at, alist, blist, fx = _pppm_handle(deck, mode, mesh, order)
        entry = fx.pppm_forces_device
    n = at.nlocal
    ele = at.echeck != 0
    q_solved = at.q.copy()
    at.q[ele] = 0.0                                    # the update has every electrode charge to write
    d_x, d_q = _to_device(at)
    pre = np.random.default_rng(5).normal(size=(n, 3))                  # (the forces of the step so far)
    d_f = torch.from_numpy(pre.copy()).cuda()
    d_ev = torch.zeros(7, dtype=torch.float64, device="cuda")
    d_e = torch.zeros(n, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    fx.pre_force_device(d_x.data_ptr(), d_q.data_ptr(), s.potdiff)
    entry(d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), d_ev.data_ptr(), d_e.data_ptr())
    torch.cuda.synchronize()
    at.q[:] = d_q.cpu().numpy()
    assert np.abs(at.q[ele] - q_solved[ele]).max() <= 1e-8 * np.abs(q_solved[ele]).max()     # (the update ran: smoke()'s bound)
    if provider == "ewald":
        want = _ewald_reference(fx, s, np.ascontiguousarray(at.x[:n]), np.ascontiguousarray(at.q[:n]))
    else:
        want = _pppm_reference(oracle, s, at, MESH0[2], MESH0[3])
    # forces at zero electrode charges are far outside the bound: the entry read what the update wrote
    _check(f"{provider}: update, then forces", (d_f.cpu().numpy() - pre, d_ev.cpu().numpy(), d_e.cpu().numpy()), want)
    fx.close()


# ---- (6) PPPM against the mesh reference -----------------------------------------------------------------------------------
def run_pppm_reference(row):
    c = pppm_case(row)
    n0 = c.fx.info().pppm_elyte_spreads
    _check(c.tag, _call(c.fx.pppm_forces_device, c.d_x, c.d_q, c.n), c.want, c.probes)
    _call(c.fx.pppm_forces_device, c.d_x, c.d_q, c.n, times=2)
    assert c.fx.info().pppm_elyte_spreads == n0 + 3          # one spread per call


@pytest.mark.parametrize("row", [pref.ROWS[0], pref.ROWS[-1]], ids=lambda r: f"{r[0]}-{r[1]}-order{r[3]}")
def test_pppm_matches_the_mesh_reference(row):
    assert {pref.ROWS[0][1], pref.ROWS[-1][1]} == {"ffield", "slab"}
    run_pppm_reference(row)


def test_pppm_never_uses_a_kept_brick(oracle):
    import copy
    import torch
    deck, mode, mesh, order = MESH0
    s, at, alist, blist, fx = _pppm_handle(deck, mode, mesh, order)
    n = at.nlocal
    fx.pppm_keep_density(True)
    fx.b_cal(at)                                       # an update: its electrolyte brick stays on the device
    d_x, d_q = _to_device(at)
    ely = np.nonzero((at.echeck[:n] == 0) & (at.q[:n] != 0))[0]
    moved = copy.copy(at)
    moved.x = at.x.copy()
    moved.x[ely[3]] += np.array([0.31, -0.27, 0.22])
    d_x[int(ely[3])] = torch.from_numpy(moved.x[ely[3]]).cuda()        # moved in the device array only
    torch.cuda.synchronize()
    want = _pppm_reference(oracle, s, moved, mesh, order)
    stale = _pppm_reference(oracle, s, at, mesh, order)
    assert np.abs(want[0] - stale[0]).max() > 1e-6 * np.abs(want[0]).max()
    _check("moved in the device array, brick kept", _call(fx.pppm_forces_device, d_x, d_q, n), want)
    fx.close()


# ---- (7) refusals; the host entries afterwards -----------------------------------------------------------------------------
def test_refusals_and_the_host_entries_after_a_device_entry(oracle):
    ce, cp = ewald_case("dilute", "ffield"), pppm_case(MESH0)
    with pytest.raises(ConpError) as e:
        cp.fx.ewald_forces_device(cp.d_x.data_ptr(), cp.d_q.data_ptr(), 0, 0, 0)
    assert e.value.code == -2 and "conp_pppm_compute" in str(e.value)                      # CONP_ERR_STATE, need_ewald's message
    with pytest.raises(ConpError) as e:
        ce.fx.pppm_forces_device(ce.d_x.data_ptr(), ce.d_q.data_ptr(), 0, 0, 0)
    assert e.value.code == -2 and "pppm/conp" in str(e.value)                              # need_pppm's message
    for c, entry in ((ce, ce.fx.ewald_forces_device), (cp, cp.fx.pppm_forces_device)):
        with pytest.raises(ConpError) as e:
            entry(0, c.d_q.data_ptr(), 0, 0, 0)
        assert e.value.code == -1                                                          # CONP_ERR_ARG
    # The host entries form what they need again: no stale cache behind a device entry.  The device entry is given OTHER charges
    # than the host's atoms carry, so whatever it leaves in the shared scratch is wrong for them.
    i = int(np.nonzero(ce.at.q[:ce.n] != 0)[0][5])
    ce.fx.ewald_compute(ce.at)                         # (a cache exists ...)
    u0 = ce.fx.ewald_particle_potential(ce.at, i)
    _call(ce.fx.ewald_forces_device, ce.d_x, ce.d_q * 1.5, ce.n)         # (... and is dropped here: the scratch is overwritten)
    assert ce.fx.ewald_particle_potential(ce.at, i) == pytest.approx(u0, rel=1e-11)
    _call(ce.fx.ewald_forces_device, ce.d_x, ce.d_q * 1.5, ce.n)
    gf, gE, gW, ge = ce.fx.ewald_forces(ce.at, eatom=True)
    _check("host ewald_forces after the device entry", (gf, np.concatenate([[gE], gW]), ge), ce.want, ce.probes)
    cp.fx.pppm_compute(cp.at)
    u0 = cp.fx.pppm_particle_potential(cp.at, i)
    _call(cp.fx.pppm_forces_device, cp.d_x, cp.d_q * 1.5, cp.n)
    assert cp.fx.pppm_particle_potential(cp.at, i) == pytest.approx(u0, rel=1e-9)         # (the spread's atomic adds: no fixed order)
    _call(cp.fx.pppm_forces_device, cp.d_x, cp.d_q * 1.5, cp.n)
    gf, gE, gW, ge = cp.fx.pppm_compute_forces(cp.at, eatom=True)
    _check("host pppm_forces after the device entry", (gf, np.concatenate([[gE], gW]), ge), cp.want, cp.probes)


# ---- (8) guard zones -------------------------------------------------------------------------------------------------------
CHILD = r'''
import sys
sys.path[:0] = [{tests!r}, {pkg!r}, {oracle!r}, {root!r}]
import torch
torch.cuda.init()
import pppm_force_ref as pref
import test_gpu_kspace_device as t
from conp_amd import capi
lib = capi.load_library()
lib.conp_debug_check_guards.restype = int
assert lib.conp_debug_check_guards() == 0, "guard zones are off"
for name, mode in (("small", "slab"), ("small", "ffield"), ("dilute", "ffield")):
    t.run_ewald_definitions(name, mode)
t.run_ewald_blocks()
for row in (pref.ROWS[0], pref.ROWS[-1]):
    t.run_pppm_reference(row)
bad = lib.conp_debug_check_guards()
assert bad == 0, (bad, lib.conp_last_error().decode())
print("GUARD_OK")
'''


def test_no_store_outside_the_buffers(tmp_path):
    script = tmp_path / "guard_child.py"
    script.write_text(CHILD.format(tests=os.path.join(ROOT, "tests"), pkg=os.path.join(ROOT, "lammps-user-conp2_amd"),
                                   oracle=os.path.join(ROOT, "oracle"), root=ROOT))
    env = dict(os.environ, CONP_GUARD="1")
    p = subprocess.run([sys.executable, str(script)], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    assert "GUARD_OK" in p.stdout
