"""The SHAKE constraint force from device arrays, beside the route an engine has without the entry.

    python tools/shake_time.py [--reps N] [--warmup W]

The headline box of bench.py (4096 electrode + 32768 electrolyte atoms): the electrolyte as 10922 three-atom clusters of flag 1 (two
bonds and the angle: the rigid cation of the IL decks, masses 67.07 / 15.04 / 57.12, 2.7076 and 3.8213 A, 116.035 degrees), every
coordinate up to 0.05 A off the ideal geometry, velocities thermal at 298 K, dt = 2 fs, tolerance 1e-4, 10 iterations at most.
After W warm-up calls each, N calls enqueued back to back with ONE synchronisation behind the last (wall = (enqueue + the final
wait) / N, host = the enqueue loop alone / N):
  - conp_shake_post_force_device without outputs (one launch), with d_out (two), with d_out and d_vatom;
  - conp_shake_setup_device, conp_shake_correct_device, conp_shake_check_device;
  - the host route the entry replaces: x, v and f down, the numpy restatement of tests/shake_ref.py, f up.
d_f is restored from a device copy inside every timed call of the force entries (a device-to-device copy of 0.9 MB on the same
stream, timed alone as ms_restore_f_wall), so that the forces stay those of the input instead of growing by a constraint force per call.
Prints one JSON line.  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import sys
import time
from types import SimpleNamespace

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lammps-user-conp2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

FTM2V = 1.0 / 48.88821291 / 48.88821291
MVV2E = 48.88821291 * 48.88821291
BOLTZ = 0.0019872067
MASS = np.array([67.07, 15.04, 57.12])
BOND_D = np.array([2.7076, 3.8213])
THETA0 = np.deg2rad(116.035)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("shake_time.py: no GPU")
    torch.cuda.init()
    from conp_amd import FixConp, capi, neighbor
    from bonded_time import timed
    from pppm_force_time import box
    import shake_ref as sr
    s, _mesh, _order = box("headline")
    at, _alist, _blist = neighbor.build_lists(s)
    n = at.nlocal
    el = np.nonzero(at.echeck[:n] == 0)[0]
    mol = el[:len(el) // 3 * 3].reshape(-1, 3)                   # centre, first and second partner
    ncl = len(mol)
    rng = np.random.default_rng(23)
    u = rng.normal(size=(ncl, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    w = np.cross(u, rng.normal(size=(ncl, 3))); w /= np.linalg.norm(w, axis=1)[:, None]
    x = at.x[:n].copy()
    x[mol[:, 1]] = x[mol[:, 0]] + BOND_D[0] * u
    x[mol[:, 2]] = x[mol[:, 0]] + BOND_D[1] * (np.cos(THETA0) * u + np.sin(THETA0) * w)
    x[mol.ravel()] += rng.uniform(-0.05, 0.05, (3 * ncl, 3))
    prd = np.where(s.periodic, s.prd, 0.0)
    for c in range(3):
        if prd[c] > 0:
            x[:, c] = s.boxlo[c] + np.mod(x[:, c] - s.boxlo[c], prd[c])
    typ = np.ones(n, dtype=np.int32)
    typ[mol[:, 1]] = 2; typ[mol[:, 2]] = 3
    one = np.ones(ncl, dtype=np.int32)
    cluster = np.stack([one, mol[:, 0], mol[:, 1], mol[:, 2], one, 2 * one, one], axis=1).astype(np.int32)
    angle_d = capi.shake_angle_distance(BOND_D[0], BOND_D[1], THETA0)
    v = rng.normal(size=(n, 3)) * np.sqrt(BOLTZ * 298.0 / (MASS[typ - 1] * MVV2E))[:, None]
    f = rng.normal(size=(n, 3)) * 10.0
    dt, tol, max_iter = 2.0, 1e-4, 10
    fx = FixConp(s)
    fx.shake_set_params(typ, MASS, BOND_D, [angle_d], cluster, tol, max_iter, dt, FTM2V, prd)
    d_x, d_v, d_f0 = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (x, v, f))
    d_f, d_xc = d_f0.clone(), d_x.clone()
    d_out = torch.zeros(9, dtype=torch.float64, device="cuda")
    d_two = torch.zeros(2, dtype=torch.float64, device="cuda")
    d_va = torch.zeros((n, 6), dtype=torch.float64, device="cuda")
    fx.set_stream(torch.cuda.current_stream().cuda_stream)      # the restoring copy and the entries on ONE stream
    X, V, F, O, VA, T = (t.data_ptr() for t in (d_x, d_v, d_f, d_out, d_va, d_two))
    sync = torch.cuda.synchronize
    rec = dict(box="headline", n_owned=int(n), n_clusters=int(ncl), reps=args.reps, warmup=args.warmup)

    def restoring(call):
        def run():
            d_f.copy_(d_f0)
            call()
        return run
    calls = {
        "restore_f": lambda: d_f.copy_(d_f0),
        "post_force": restoring(lambda: fx.shake_post_force_device(X, V, F, 0, 0)),
        "post_force_with_d_out": restoring(lambda: fx.shake_post_force_device(X, V, F, O, 0)),
        "post_force_with_d_out_and_vatom": restoring(lambda: fx.shake_post_force_device(X, V, F, O, VA)),
        "setup_with_d_out": restoring(lambda: fx.shake_setup_device(X, V, F, O)),
        "check": lambda: fx.shake_check_device(X, T),
        "correct": lambda: fx.shake_correct_device(d_xc.data_ptr()),
    }
    for name, call in calls.items():
        rec[f"ms_{name}_wall"], rec[f"ms_{name}_host_thread"] = timed(call, args.reps, args.warmup, sync)
    out = d_out.cpu().numpy()
    rec["unconverged"], rec["bad_determinants"], rec["largest_niter"] = int(out[6]), int(out[7]), int(out[8])
    rec["deviation_before"] = [float(q) for q in d_two.cpu().numpy()]
    fx.shake_check_device(d_xc.data_ptr(), T)
    rec["deviation_after_correct"] = [float(q) for q in d_two.cpu().numpy()]

    # the route without the entry: x, v and f down, the float64 restatement of the rule in numpy, f up
    case = SimpleNamespace(type=typ, mass=MASS, bond_d=BOND_D, angle_d=np.array([angle_d]), cluster=cluster, tolerance=tol,
                           max_iter=max_iter, dt=dt, ftm2v=FTM2V, prd=prd)
    rule = sr.Rule("f64", case)
    d_f.copy_(d_f0)
    fx.shake_post_force_device(X, V, F, 0, 0)
    f_dev = d_f.cpu().numpy()

    def host_route():
        hx, hv, hf = d_x.cpu().numpy(), d_v.cpu().numpy(), d_f0.cpu().numpy()
        res = rule.solve(hx, hv, hf)
        d_f.copy_(torch.from_numpy(res.out))
        return res
    rec["ms_host_route"], _ = timed(host_route, max(args.reps // 20, 5), 2, sync)
    rec["device_equals_host_restatement"] = bool(host_route().out.tobytes() == f_dev.tobytes())
    t0 = time.perf_counter()
    d_x.cpu(); d_v.cpu(); d_f0.cpu(); d_f.copy_(torch.from_numpy(f_dev)); sync()
    rec["ms_host_route_copies_alone"] = round(1e3 * (time.perf_counter() - t0), 4)
    print(json.dumps(rec), flush=True)
    fx.close()


if __name__ == "__main__":
    main()
