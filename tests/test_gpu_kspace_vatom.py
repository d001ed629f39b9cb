"""-m gpu: the per-atom virial of the k-space force entries -- conp_ewald_compute_forces_vatom, conp_pppm_compute_forces_vatom and
their _device twins.

(1) Ewald host and device entries against the numpy definitions of tests/kspace_vatom_ref.py, zero-charge probes exact zeros, the
    other outputs of the same call against the siblings' references, sum_i vatom_i against the call's own virial;  (2) blocks of 64
    with a ragged last one;  (3) PPPM host and device entries on the four ROWS meshes against the numpy mesh reference (six separate
    transforms) and against the exact sum within twice VATOM_MEASURED;  (4) vatom = NULL is the sibling (bitwise for Ewald);
    (5) vatom alone;  (6) NaN pre-fill overwritten, three calls with one synchronisation;  (7) an update followed by the entry;
    (8) refusals;  (9) guard zones.
Bounds: 1e-11 of the unsubtracted scale (qs sum ug |S|^2, or qs (V / 2) sum G |rho^|^2 / N^2) for every vatom entry; the siblings'
bounds (tests/test_gpu_kspace_device.py) for the other outputs.  sum_i vatom_i against the returned virial: 1e-13 of the scale -- a
hundredth of the bound, not its nlocal^1/2 multiple: measured on an MI355X the sums agree to 3.2e-4 of the 1e-11 bound at most
(il_onelayer, 3776 atoms; 6e-5 and less elsewhere), see DESIGN.md section 15 for the fractions per case."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import ewald_force_ref as eref
import kspace_vatom_ref as vref
import pppm_force_ref as pref
from conp_amd import ConpError, capi
from test_gpu_kspace_device import MESH0, _check, _compare, _to_device, ewald_case, pppm_case
from test_gpu_ewald_potential import _handle as _ewald_handle, _system
from test_gpu_pppm_forces import _handle as _pppm_handle

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EWALD_CASES = [("small", "slab"), ("small", "ffield"), ("dilute", "ffield")]


def _vcall(entry, d_x, d_q, n, f=True, ev=True, eatom=True, vatom=True, times=1):
    """`times` calls of a _vatom_device entry, NO synchronisation between them, one afterwards -> (f, ev, e, v); overwritten
    outputs start as NaN"""
    import torch
    d_f = torch.zeros((n, 3), dtype=torch.float64, device="cuda") if f else None
    d_ev = torch.full((7,), float("nan"), dtype=torch.float64, device="cuda") if ev else None
    d_e = torch.full((n,), float("nan"), dtype=torch.float64, device="cuda") if eatom else None
    d_v = torch.full((n, 6), float("nan"), dtype=torch.float64, device="cuda") if vatom else None
    torch.cuda.synchronize()
    for _ in range(times):
        entry(d_x.data_ptr(), d_q.data_ptr(), *(0 if t is None else t.data_ptr() for t in (d_f, d_ev, d_e, d_v)))
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (d_f, d_ev, d_e, d_v))


def _xq(c):
    return np.ascontiguousarray(c.at.x[:c.n]), np.ascontiguousarray(c.at.q[:c.n])


@functools.lru_cache(maxsize=None)
def ewald_vatom_want(name, mode):
    c = ewald_case(name, mode)
    T = eref.handle_tables(c.fx, c.s)
    x, q = _xq(c)
    S = eref.structure_factor(x, q, T["kv"])
    return vref.ewald_vatom(S, x, q, T["kv"], T["ug"], T["g"], T["qs"], np.arange(c.n))


@functools.lru_cache(maxsize=None)
def pppm_vatom_want(row):
    import oracle_py
    c = pppm_case(row)
    v, W, scale, T, x, q = vref.reference(oracle_py.load(), c.s, c.at, c.mesh, c.order)
    return v, vref.exact_vatom(c.s, x, q, T, np.arange(c.n))


def _check_vatom(tag, v, want, virial, scale, probes):
    assert v.shape == want.shape and np.all(np.isfinite(v))              # (the NaN pre-fill is gone)
    assert np.all(v[probes] == 0.0) and np.abs(want).max() > 0
    _compare(f"{tag} vatom", v, want, 1e-11 * scale)
    if virial is not None:
        _compare(f"{tag} sum_i vatom_i against the call's virial", v.sum(axis=0), virial, 1e-13 * scale)


# ---- (1) Ewald against the definitions -------------------------------------------------------------------------------------
def run_ewald_definitions(name, mode):
    c = ewald_case(name, mode)
    want, scale = ewald_vatom_want(name, mode), c.want[4]
    f, ev, e, v = _vcall(c.fx.ewald_forces_vatom_device, c.d_x, c.d_q, c.n)
    _check(f"{c.tag} device", (f, ev, e), c.want, c.probes)
    _check_vatom(f"{c.tag} device", v, want, ev[1:], scale, c.probes)
    c.fx.ewald_compute(c.at)                           # S of THESE atoms (the probes were made after the handle's update)
    f, E, W, e, v = c.fx.ewald_forces_vatom(c.at, eatom=True)
    _check(f"{c.tag} host", (f, np.concatenate([[E], W]), e), c.want, c.probes)
    _check_vatom(f"{c.tag} host", v, want, W, scale, c.probes)


@pytest.mark.parametrize("name,mode", EWALD_CASES)
def test_ewald_vatom_matches_the_definitions(name, mode):
    run_ewald_definitions(name, mode)


# ---- (2) blocks of 64, a ragged last one -----------------------------------------------------------------------------------
def run_ewald_blocks():
    c = ewald_case("dilute", "ffield")
    assert c.n > 2 * 64 and c.n % 64 != 0, c.n
    want, scale = ewald_vatom_want("dilute", "ffield"), c.want[4]
    one = _vcall(c.fx.ewald_forces_vatom_device, c.d_x, c.d_q, c.n)
    capi.set_ew_block(64)
    try:
        got = _vcall(c.fx.ewald_forces_vatom_device, c.d_x, c.d_q, c.n)
        c.fx.ewald_compute(c.at)
        host = c.fx.ewald_forces_vatom(c.at, eatom=True)
    finally:
        capi.set_ew_block(0)
    tag = f"{c.tag}, blocks of 64 ({c.n} atoms: {c.n // 64} full + {c.n % 64})"
    _check(tag, got[:3], c.want, c.probes)
    _check_vatom(tag, got[3], want, got[1][1:], scale, c.probes)
    _compare(f"{tag} against one block", got[3], one[3], 1e-11 * scale)
    _check_vatom(f"{tag} host", host[4], want, host[2], scale, c.probes)


def test_ewald_vatom_in_blocks_with_a_ragged_last_block():
    run_ewald_blocks()


# ---- (3) PPPM against the mesh reference and the exact sum -----------------------------------------------------------------
def run_pppm_reference(row):
    c = pppm_case(row)
    (want, exact), scale = pppm_vatom_want(row), c.want[4]
    f, ev, e, v = _vcall(c.fx.pppm_forces_vatom_device, c.d_x, c.d_q, c.n)
    _check(f"{c.tag} device", (f, ev, e), c.want, c.probes)
    _check_vatom(f"{c.tag} device", v, want, ev[1:], scale, c.probes)
    hf, E, W, he, hv = c.fx.pppm_forces_vatom(c.at, eatom=True)
    _check(f"{c.tag} host", (hf, np.concatenate([[E], W]), he), c.want, c.probes)
    _check_vatom(f"{c.tag} host", hv, want, W, scale, c.probes)
    for tag, got in (("device", v), ("host", hv)):
        err = vref.rms_all(got - exact) / vref.rms_all(exact)
        print(f"{c.tag} {tag}: vatom against the exact sum {err:.3e} (recorded for the reference: {vref.VATOM_MEASURED[row]:.3e})")
        assert err <= 2 * vref.VATOM_MEASURED[row]


@pytest.mark.parametrize("row", pref.ROWS, ids=lambda r: f"{r[0]}-{r[1]}-{'x'.join(map(str, r[2]))}-order{r[3]}")
def test_pppm_vatom_matches_the_mesh_reference_and_the_exact_sum(row):
    run_pppm_reference(row)


# ---- (4) vatom = NULL is the sibling ---------------------------------------------------------------------------------------
def test_ewald_without_vatom_returns_the_siblings_bits():
    from test_gpu_kspace_device import _call
    c = ewald_case("dilute", "ffield")
    old = _call(c.fx.ewald_forces_device, c.d_x, c.d_q, c.n)
    new = _vcall(c.fx.ewald_forces_vatom_device, c.d_x, c.d_q, c.n, vatom=False)
    withv = _vcall(c.fx.ewald_forces_vatom_device, c.d_x, c.d_q, c.n)
    for a, b, w in zip(old, new[:3], withv[:3]):
        assert np.array_equal(a, b) and np.array_equal(a, w)           # (asking for vatom does not move the other outputs either)
    c.fx.ewald_compute(c.at)
    ho = c.fx.ewald_forces(c.at, eatom=True)
    hn = c.fx.ewald_forces_vatom(c.at, eatom=True, vatom=False)
    assert hn[4] is None
    for a, b in zip(ho, hn[:4]):
        assert np.array_equal(np.asarray(a), np.asarray(b))


def test_pppm_without_vatom_agrees_with_the_sibling():
    """to the rounding the spread's atomic adds allow: 1e-4 of the bounds (section 14 measured 3e-5)"""
    from test_gpu_kspace_device import _call
    c = pppm_case(MESH0)
    scale, fmax = c.want[4], np.abs(c.want[0]).max()
    old = _call(c.fx.pppm_forces_device, c.d_x, c.d_q, c.n)
    new = _vcall(c.fx.pppm_forces_vatom_device, c.d_x, c.d_q, c.n, vatom=False)
    _compare("pppm device, vatom NULL: force", new[0], old[0], 1e-4 * 1e-10 * fmax)
    _compare("pppm device, vatom NULL: energy and virial", new[1], old[1], 1e-4 * 1e-11 * scale)
    _compare("pppm device, vatom NULL: eatom", new[2], old[2], 1e-4 * 1e-11 * scale)
    ho = c.fx.pppm_compute_forces(c.at, eatom=True)
    hn = c.fx.pppm_forces_vatom(c.at, eatom=True, vatom=False)
    _compare("pppm host, vatom NULL: force", hn[0], ho[0], 1e-4 * 1e-10 * fmax)
    _compare("pppm host, vatom NULL: energy", hn[1], ho[1], 1e-4 * 1e-11 * scale)
    _compare("pppm host, vatom NULL: virial", hn[2], ho[2], 1e-4 * 1e-11 * scale)
    _compare("pppm host, vatom NULL: eatom", hn[3], ho[3], 1e-4 * 1e-11 * scale)


# ---- (5) vatom alone; (6) overwritten, three calls and one synchronisation --------------------------------------------------
@pytest.mark.parametrize("provider", ["ewald", "pppm"])
def test_vatom_alone_and_three_calls_with_one_synchronisation(provider):
    if provider == "ewald":
        c = ewald_case("dilute", "ffield")
        want, dev, host = ewald_vatom_want("dilute", "ffield"), c.fx.ewald_forces_vatom_device, c.fx.ewald_forces_vatom
    else:
        c = pppm_case(MESH0)
        want, dev, host = pppm_vatom_want(MESH0)[0], c.fx.pppm_forces_vatom_device, c.fx.pppm_forces_vatom
    scale = c.want[4]
    n0 = c.fx.info().pppm_elyte_spreads
    dev(c.d_x.data_ptr(), c.d_q.data_ptr(), 0, 0, 0, 0)                 # all four NULL: CONP_OK, nothing done
    assert c.fx.info().pppm_elyte_spreads == n0
    got = _vcall(dev, c.d_x, c.d_q, c.n, f=False, ev=False, eatom=False)
    assert got[:3] == (None, None, None)
    _check_vatom(f"{provider} device, vatom alone", got[3], want, None, scale, c.probes)
    if provider == "ewald":
        c.fx.ewald_compute(c.at)
    h = host(c.at, energy=False, virial=False, eatom=False, forces=False)
    assert h[:4] == (None, None, None, None)
    _check_vatom(f"{provider} host, vatom alone", h[4], want, None, scale, c.probes)
    f3, ev3, e3, v3 = _vcall(dev, c.d_x, c.d_q, c.n, times=3)
    _check_vatom(f"{provider} device, three calls", v3, want, ev3[1:], scale, c.probes)
    _compare(f"{provider} device, three calls: forces accumulate", f3, 3 * c.want[0], 3e-10 * np.abs(c.want[0]).max())


# ---- (7) an update followed by the entry, nothing between them -------------------------------------------------------------
@pytest.mark.parametrize("provider", ["ewald", "pppm"])
def test_an_update_then_the_entry(provider, oracle):
    import torch
    if provider == "ewald":
        s = _system("dilute", "ffield")
        at, alist, blist, fx = _ewald_handle(s)
        entry = fx.ewald_forces_vatom_device
    else:
        deck, mode, mesh, order = MESH0
        s, at, alist, blist, fx = _pppm_handle(deck, mode, mesh, order)
        entry = fx.pppm_forces_vatom_device
    n = at.nlocal
    ele = at.echeck != 0
    q_solved = at.q.copy()
    at.q[ele] = 0.0                                    # the update has every electrode charge to write
    d_x, d_q = _to_device(at)
    d_ev = torch.full((7,), float("nan"), dtype=torch.float64, device="cuda")
    d_v = torch.full((n, 6), float("nan"), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    fx.pre_force_device(d_x.data_ptr(), d_q.data_ptr(), s.potdiff)
    entry(d_x.data_ptr(), d_q.data_ptr(), 0, d_ev.data_ptr(), 0, d_v.data_ptr())
    torch.cuda.synchronize()
    at.q[:] = d_q.cpu().numpy()
    assert np.abs(at.q[ele] - q_solved[ele]).max() <= 1e-8 * np.abs(q_solved[ele]).max()
    x, q = np.ascontiguousarray(at.x[:n]), np.ascontiguousarray(at.q[:n])
    if provider == "ewald":
        T = eref.handle_tables(fx, s)
        S = eref.structure_factor(x, q, T["kv"])
        want, scale = vref.ewald_vatom(S, x, q, T["kv"], T["ug"], T["g"], T["qs"], np.arange(n)), T["qs"] * eref.ksum(S, T["ug"])
    else:
        want, W, scale, T, x, q = vref.reference(oracle, s, at, MESH0[2], MESH0[3])
    ev = d_ev.cpu().numpy()
    _check_vatom(f"{provider}: update, then vatom", d_v.cpu().numpy(), want, ev[1:], scale, np.zeros(0, int))
    fx.close()


# ---- (8) refusals ----------------------------------------------------------------------------------------------------------
def test_the_siblings_refusals_apply():
    ce, cp = ewald_case("dilute", "ffield"), pppm_case(MESH0)
    with pytest.raises(ConpError) as e:
        cp.fx.ewald_forces_vatom_device(cp.d_x.data_ptr(), cp.d_q.data_ptr(), 0, 0, 0, 0)
    assert e.value.code == -2 and "conp_pppm_compute" in str(e.value)
    with pytest.raises(ConpError) as e:
        ce.fx.pppm_forces_vatom_device(ce.d_x.data_ptr(), ce.d_q.data_ptr(), 0, 0, 0, 0)
    assert e.value.code == -2 and "pppm/conp" in str(e.value)
    with pytest.raises(ConpError) as e:
        cp.fx.ewald_forces_vatom(cp.at)
    assert e.value.code == -2
    with pytest.raises(ConpError) as e:
        ce.fx.pppm_forces_vatom(ce.at)
    assert e.value.code == -2 and "conp_ewald_compute_forces_vatom" in str(e.value)
    for c, entry in ((ce, ce.fx.ewald_forces_vatom_device), (cp, cp.fx.pppm_forces_vatom_device)):
        with pytest.raises(ConpError) as e:
            entry(0, c.d_q.data_ptr(), 0, 0, 0, 0)
        assert e.value.code == -1


# ---- (9) guard zones -------------------------------------------------------------------------------------------------------
CHILD = r'''
import sys
sys.path[:0] = [{tests!r}, {pkg!r}, {oracle!r}, {root!r}]
import torch
torch.cuda.init()
import pppm_force_ref as pref
import test_gpu_kspace_vatom as t
from conp_amd import capi
lib = capi.load_library()
lib.conp_debug_check_guards.restype = int
assert lib.conp_debug_check_guards() == 0, "guard zones are off"
t.run_ewald_definitions("small", "slab")
t.run_ewald_definitions("dilute", "ffield")
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
