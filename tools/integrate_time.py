"""The two halves of a velocity-Verlet step with a Nose-Hoover chain from device arrays, beside the pair and bonded entries' time in
the same process and the route an engine has without them.

    python tools/integrate_time.py [--reps N] [--warmup W]

The headline box of bench.py (4096 electrode + 32768 electrolyte atoms, ffield): 36864 owned atoms, the electrolyte one nvt group at
298 K with Tdamp 100 fs, the electrode in no group.  After W warm-up calls each, N calls enqueued back to back with ONE
synchronisation behind the last (wall = (enqueue + the final wait) / N, host = the enqueue loop alone / N):
  - conp_integrate_initial_device and conp_integrate_final_device (with and without d_out) alone, and the two in turn as a step;
  - conp_integrate_temperature_device;
  - for scale conp_pair_compute_device (forces only) and conp_bonded_compute_device (forces only) on the same atoms, as
    tools/bonded_time.py sets them up;
  - the host route: v and f down, one numpy half-step with the temperature sum and the chain on the host, x and v up -- twice
    per step.
Prints one JSON line.  Needs a GPU: there is no fall-back."""
import argparse
import dataclasses
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lammps-user-conp2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

FTM2V = 1.0 / 48.88821291 / 48.88821291
MVV2E = 48.88821291 * 48.88821291
BOLTZ = 0.0019872067
MASS = np.array([67.07, 15.04, 57.12, 144.96, 12.001])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("integrate_time.py: no GPU")
    torch.cuda.init()
    from conp_amd import FixConp, neighbor
    from bonded_time import molecules, timed
    from pair_time import lj_tables
    from pppm_force_time import box, charge_electrodes
    s, _mesh, _order = box("headline")
    at, alist, blist = neighbor.build_lists(s)
    charge_electrodes(at)
    pairs = neighbor.build_lists(dataclasses.replace(s, eletypes=None))[1]
    nall, n = at.nall, at.nlocal
    fx = FixConp(s)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.pair_set_params(s.cutsq_table(), s.cutoff, lj_tables(s.ntypes, s.cutoff))
    fx.pair_set_list(pairs, nall)
    xm, bonds, angles = molecules(s)
    xb = at.x.copy(); xb[:n] = xm
    fx.bonded_set_params([450.0], [1.0], [55.0], [np.deg2rad(104.52)], newton_bond=True)
    fx.bonded_set_lists(n, nall, bonds, angles, np.where(s.periodic, s.prd, 0.0))
    # the integrator: the electrolyte is group 0 (nvt), the electrode -1
    elyte = at.echeck[:n] == 0
    group = np.where(elyte, 0, -1).astype(np.int32)
    mass = np.resize(MASS, s.ntypes)
    m_atom = mass[at.type[:n] - 1]
    rng = np.random.default_rng(5)
    v0 = rng.normal(size=(nall, 3)) * 1e-3
    v0[:n] = rng.normal(size=(n, 3)) * np.sqrt(BOLTZ * 298.0 / (m_atom * MVV2E))[:, None]
    f0 = rng.normal(size=(nall, 3)) * 1e-3         # small, so that hundreds of steps without a force evaluation stay finite
    dof = np.array([3.0 * elyte.sum() - 3.0])
    t_target = np.array([298.0])
    dt = 1.0
    fx.integrate_set_params(at.type[:n], group, mass, [1], dof, [100.0], dt, FTM2V, MVV2E, BOLTZ)
    d_x = torch.from_numpy(np.ascontiguousarray(at.x)).cuda()
    d_xb = torch.from_numpy(np.ascontiguousarray(xb)).cuda()
    d_xi = d_x.clone()
    d_q = torch.from_numpy(at.q.copy()).cuda()
    d_v = torch.from_numpy(v0.copy()).cuda()
    d_f = torch.from_numpy(f0.copy()).cuda()
    d_fo = torch.zeros((nall, 3), dtype=torch.float64, device="cuda")
    d_out = torch.zeros((1, 4), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    fx.integrate_setup_device(d_v.data_ptr(), t_target)
    X, V, F, O = d_xi.data_ptr(), d_v.data_ptr(), d_f.data_ptr(), d_out.data_ptr()
    sync = torch.cuda.synchronize
    rec = dict(box="headline", n_owned=int(n), n_integrated=int(elyte.sum()), reps=args.reps, warmup=args.warmup)
    calls = {
        "initial": lambda: fx.integrate_initial_device(X, V, F, t_target),
        "final": lambda: fx.integrate_final_device(V, F, 0),
        "final_with_d_out": lambda: fx.integrate_final_device(V, F, O),
        "temperature": lambda: fx.integrate_temperature_device(V, O),
    }
    for name, call in calls.items():
        rec[f"ms_{name}_wall"], rec[f"ms_{name}_host_thread"] = timed(call, args.reps, args.warmup, sync)

    def step():
        fx.integrate_initial_device(X, V, F, t_target)
        fx.integrate_final_device(V, F, O)
    rec["ms_step_wall"], rec["ms_step_host_thread"] = timed(step, args.reps, args.warmup, sync)
    rec["t_current_after"] = float(d_out.cpu().numpy()[0, 0])
    rec["ms_pair_device_forces_wall"], _ = timed(
        lambda: fx.pair_compute_device(d_x.data_ptr(), d_q.data_ptr(), d_fo.data_ptr(), 0, 0, 0), max(args.reps // 10, 5), 3, sync)
    rec["ms_bonded_device_forces_wall"], _ = timed(
        lambda: fx.bonded_compute_device(d_xb.data_ptr(), d_fo.data_ptr(), 0, 0, 0), args.reps, args.warmup, sync)

    # the route without the entries: v and f down, a numpy half-step (update, temperature sum, chain, scale), x and v up
    dtf = 0.5 * dt * FTM2V
    dtfm = np.where(elyte, dtf / m_atom, 0.0)[:, None]
    chain = dict(ed=0.0)

    def host_half():
        v = d_v.cpu().numpy(); f = d_f.cpu().numpy(); x = d_xi.cpu().numpy()
        v[:n] += dtfm * f[:n]
        t = float(((v[:n] * v[:n]).sum(axis=1) * m_atom)[elyte].sum()) * MVV2E / (dof[0] * BOLTZ)
        chain["ed"] += 0.25 * dt * (t - t_target[0]) / t_target[0] * 1e-4
        v[:n][elyte] *= np.exp(-0.5 * dt * chain["ed"])
        x[:n][elyte] += dt * v[:n][elyte]
        d_v.copy_(torch.from_numpy(v)); d_xi.copy_(torch.from_numpy(x))
    rec["ms_host_route_half_step"], _ = timed(host_half, max(args.reps // 10, 5), 3, sync)
    rec["ms_host_route_step"] = round(2 * rec["ms_host_route_half_step"], 4)
    print(json.dumps(rec), flush=True)
    fx.close()


if __name__ == "__main__":
    main()
