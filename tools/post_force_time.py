"""The Gaussian correction of a step (FixConp::post_force) through host buffers and on the device, in one process (DESIGN.md
section 20).

    python tools/post_force_time.py [--reps N] [--warmup W]

The headline box of bench.py (systems.synthetic_fast defaults: 4096 electrode + 32768 electrolyte atoms, ffield), the lists of
tools/pair_time.py, the fix's list being the electrode-electrolyte skip list.  After setup and one conp_fix_pre_force at step 1, and W
warm-up calls each, N calls of
  (a) host entry     conp_fix_post_force_step at step 1 (positions and charges already on the device; the entry reads its nine
                     accumulators back and synchronises in every call): wall time per call.  The yardstick.
  (b) device entry   conp_fix_post_force_device with both outputs on device copies of the same atoms: N calls enqueued back to back,
                     ONE synchronisation behind the last; wall = (enqueue + the final wait) / N, host = the enqueue loop alone / N;
                     and the same with d_f alone (no sums, no finish kernel)
Prints one JSON line with the times, the owners and listed pairs of the fix's list and the contributing pairs (0 in this box: no
electrolyte atom sits within 1.2 A of an electrode atom, as in any normal MD step).  Needs a GPU: there is no fall-back."""
import argparse
import ctypes as C
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
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("post_force_time.py: no GPU")
    torch.cuda.init()
    from conp_amd import FixConp, capi, neighbor
    from pppm_force_time import box
    s, _mesh, _order = box("headline")
    at, alist, blist = neighbor.build_lists(s)
    nall = at.nall
    fx = FixConp(s)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)
    fx.pre_force(at, 1, s.potdiff)
    # (a) the host entry, with output arrays made once
    f = np.zeros((nall, 3)); ek = C.c_double(); ec = C.c_double(); vir = np.zeros(6)
    view = fx.atoms_view(at)
    dp = lambda a: a.ctypes.data_as(C.POINTER(C.c_double))

    def host():
        fx._check(fx.lib.conp_fix_post_force_step(fx.h, C.byref(view), C.c_int64(1), dp(f), C.byref(ek), C.byref(ec), dp(vir)))
    for _ in range(args.warmup):
        host()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        host()
    ms_host = 1e3 * (time.perf_counter() - t0) / args.reps
    # (b) the device entry
    d_x = torch.from_numpy(np.ascontiguousarray(at.x)).cuda()
    d_q = torch.from_numpy(at.q.copy()).cuda()
    d_f = torch.zeros((nall, 3), dtype=torch.float64, device="cuda")
    d_out = torch.zeros(9, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()

    def timed(with_out):
        def device():
            fx.post_force_device(d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), d_out.data_ptr() if with_out else 0)
        for _ in range(args.warmup):
            device()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            device()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        return t0, t1, time.perf_counter()
    f0, f1, f2 = timed(False)                    # forces only: the pair kernel without its sums, no finish kernel
    t0, t1, t2 = timed(True)
    out = d_out.cpu().numpy()
    rec = dict(box="headline", n_owned=int(at.nlocal), n_all=int(nall), list_owners=int(blist.inum), listed_pairs=int(blist.npairs),
               contributing_pairs=float(out[8]), reps=args.reps, warmup=args.warmup,
               ms_host_post_force_step=round(ms_host, 4),
               ms_device_wall=round(1e3 * (t2 - t0) / args.reps, 4), ms_device_host_thread=round(1e3 * (t1 - t0) / args.reps, 4),
               ms_device_forces_only_wall=round(1e3 * (f2 - f0) / args.reps, 4),
               self_energy_equal=bool(out[0] == ek.value))
    print(json.dumps(rec), flush=True)
    fx.close()


if __name__ == "__main__":
    main()
