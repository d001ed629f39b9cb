"""The k-space force half of a step from host arrays and from device arrays, in one process.

    python tools/kspace_device_time.py [--reps N] [--warmup W] [--vatom]

Two boxes (il_onelayer; the headline box of bench.py: 4096 electrode + 32768 electrolyte atoms, ffield), both providers (the exact
Ewald sum; PPPM on the meshes of tools/pppm_force_time.py).  Per box and provider, after W warm-up calls each:
  host pair      conp_ewald_compute + conp_ewald_compute_forces (Ewald) or conp_pppm_compute_forces (PPPM): host arrays in, f, energy
                 and virial out; the calls are synchronous, so the wall time per call IS the time the host thread spends in it
  device entry   conp_*_compute_forces_device on device copies of the same atoms (d_f, d_ev): N calls enqueued back to back, ONE
                 synchronisation behind the last.  wall = (enqueue + the final wait) / N; host = the enqueue loop alone / N, the time
                 the host thread spends inside the calls.  A host time near the wall time would mean the entry waits for the device.
  --vatom        also times conp_*_compute_forces_vatom_device (d_f, d_ev, d_vatom: DESIGN.md section 15) the same way, in the same
                 process behind the existing entry: ms_vatom_device_wall / ms_vatom_device_host_thread and their ratio to the entry
                 without the per-atom virial
Prints one JSON line per box and provider.  Needs a GPU: there is no fall-back."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lammps-user-conp2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--vatom", action="store_true", help="also time the entries with the per-atom virial")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("kspace_device_time.py: no GPU")
    torch.cuda.init()
    from conp_amd import FixConp, neighbor
    from pppm_force_time import box, charge_electrodes
    for name in ("il_onelayer", "headline"):
        s, mesh, order = box(name)
        at, alist, blist = neighbor.build_lists(s)
        charge_electrodes(at)
        n = at.nlocal
        f = np.zeros((n, 3))
        d_x = torch.from_numpy(np.ascontiguousarray(at.x)).cuda()
        d_q = torch.from_numpy(at.q.copy()).cuda()
        d_f = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
        d_ev = torch.zeros(7, dtype=torch.float64, device="cuda")
        d_v = torch.zeros((n, 6), dtype=torch.float64, device="cuda")
        for provider in ("ewald", "pppm"):
            if provider == "ewald":
                fx = FixConp(s)
            else:
                fx = FixConp(s, extra_args=["pppm"], pppm_mesh=mesh, pppm_order=order)
            fx.init_lists(alist, blist)
            fx.setup_post_neighbor(at)
            if provider == "ewald":
                def host():
                    fx.ewald_compute(at)
                    fx.ewald_forces(at, f=f)
                entry, ventry = fx.ewald_forces_device, fx.ewald_forces_vatom_device
            else:
                def host():
                    fx.pppm_compute_forces(at, f=f)
                entry, ventry = fx.pppm_forces_device, fx.pppm_forces_vatom_device

            def device():
                entry(d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), d_ev.data_ptr(), 0)

            def device_vatom():
                ventry(d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), d_ev.data_ptr(), 0, d_v.data_ptr())

            def timed(call):
                for _ in range(args.warmup):
                    call()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                for _ in range(args.reps):
                    call()
                t1 = time.perf_counter()
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                return 1e3 * (t2 - t0) / args.reps, 1e3 * (t1 - t0) / args.reps
            for _ in range(args.warmup):
                host()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                host()
            ms_host = 1e3 * (time.perf_counter() - t0) / args.reps
            ms_dev_wall, ms_dev_thread = timed(device)
            rec = dict(box=name, provider=provider, n_atoms=int(n), mesh=list(mesh) if provider == "pppm" else None,
                       kcount=int(fx.info().kcount), ms_host_pair_wall=round(ms_host, 4), ms_host_pair_host_thread=round(ms_host, 4),
                       ms_device_wall=round(ms_dev_wall, 4), ms_device_host_thread=round(ms_dev_thread, 4),
                       host_over_device=round(ms_host / ms_dev_wall, 3), reps=args.reps, warmup=args.warmup)
            if args.vatom:
                ms_v_wall, ms_v_thread = timed(device_vatom)
                rec.update(ms_vatom_device_wall=round(ms_v_wall, 4), ms_vatom_device_host_thread=round(ms_v_thread, 4),
                           vatom_over_device=round(ms_v_wall / ms_dev_wall, 3))
            print(json.dumps(rec), flush=True)
            fx.close()


if __name__ == "__main__":
    main()
