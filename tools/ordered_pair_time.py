"""The atomic-free pair and Gaussian-correction entries beside their atomic twins, in one process.

    python tools/ordered_pair_time.py [--reps N] [--warmup W]

The headline box and the synthetic LJ coefficients of tools/pair_time.py, and its method: after W warm-up calls, N calls enqueued back
to back and ONE synchronisation behind the last; wall = (enqueue + the final wait) / N.  Measured:
  atomic    conp_pair_compute_device (the kernel as it was): forces; forces, energy and virial; those with eatom and vatom
  ordered   conp_pair_compute_ordered_device, the same three
  ev_alone  conp_pair_compute_device with d_ev as its only output: what d_ev would cost the ordered entry as a second launch of the
            atomic entry's <sums, no force> instantiation instead of the row record inside the gather (ordered forces_ev - forces)
  transpose conp_pair_transpose_list_device of the pair list and conp_fix_transpose_list_device of the fix's (synchronous: wall time
            per call), beside the 0.49 ms of the list build they follow
  gaussian  conp_fix_post_force_device and conp_fix_post_force_ordered_device, d_f and d_out
and the cost per MD step at one re-neighbouring per 10 steps.  Prints one JSON line.  Needs a GPU: there is no fall-back."""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lammps-user-conp2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("ordered_pair_time.py: no GPU")
    torch.cuda.init()
    from conp_amd import FixConp, neighbor
    from pair_time import lj_tables
    from pppm_force_time import box, charge_electrodes
    s, _mesh, _order = box("headline")
    at, alist, blist = neighbor.build_lists(s)
    charge_electrodes(at)
    pairs = neighbor.build_lists(dataclasses.replace(s, eletypes=None))[1]       # the pair style's list: every pair
    nall = at.nall
    fx = FixConp(s)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)
    fx.pair_set_params(s.cutsq_table(), s.cutoff, lj_tables(s.ntypes, s.cutoff))
    fx.pair_set_list(pairs, nall)
    d_x = torch.from_numpy(np.ascontiguousarray(at.x)).cuda()
    d_q = torch.from_numpy(at.q.copy()).cuda()
    d_f = torch.zeros((nall, 3), dtype=torch.float64, device="cuda")
    d_ev = torch.zeros(8, dtype=torch.float64, device="cuda")
    d_e = torch.zeros(nall, dtype=torch.float64, device="cuda")
    d_v = torch.zeros((nall, 6), dtype=torch.float64, device="cuda")
    d_out = torch.zeros(9, dtype=torch.float64, device="cuda")
    rec = dict(box="headline", n_owned=int(at.nlocal), n_all=int(nall), cutoff=float(s.cutoff), listed_pairs=int(pairs.npairs),
               fix_listed_pairs=int(blist.npairs), reps=args.reps, warmup=args.warmup, ms_list_build_device=0.49)

    def sync_timed(call, key):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            call()
        rec[key] = round(1e3 * (time.perf_counter() - t0) / args.reps, 4)

    def stream_timed(call, key):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            call()
        torch.cuda.synchronize()
        rec[key] = round(1e3 * (time.perf_counter() - t0) / args.reps, 4)

    sync_timed(fx.pair_transpose_list_device, "ms_transpose_pair_list")
    sync_timed(fx.fix_transpose_list_device, "ms_transpose_fix_list")
    X, Q, F = d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr()
    outputs = {"forces": (F, 0, 0, 0), "forces_ev": (F, d_ev.data_ptr(), 0, 0),
               "forces_ev_atom": (F, d_ev.data_ptr(), d_e.data_ptr(), d_v.data_ptr())}
    for name, out in outputs.items():
        stream_timed(lambda: fx.pair_compute_device(X, Q, *out), f"ms_atomic_{name}")
        stream_timed(lambda: fx.pair_compute_ordered_device(X, Q, *out), f"ms_ordered_{name}")
    stream_timed(lambda: fx.pair_compute_device(X, Q, 0, d_ev.data_ptr(), 0, 0), "ms_atomic_ev_alone")
    stream_timed(lambda: fx.post_force_device(X, Q, F, d_out.data_ptr()), "ms_gaussian_atomic")
    stream_timed(lambda: fx.post_force_ordered_device(X, Q, F, d_out.data_ptr()), "ms_gaussian_ordered")
    rec["gaussian_contributing_pairs"] = float(d_out.cpu().numpy()[8])
    # faster and different is not faster: both entries once more from zeroed outputs, at the size that was timed
    got = {}
    for name, entry in (("atomic", fx.pair_compute_device), ("ordered", fx.pair_compute_ordered_device)):
        d_f.zero_()
        entry(X, Q, *outputs["forces_ev_atom"])
        torch.cuda.synchronize()
        got[name] = [t.cpu().numpy().copy() for t in (d_f, d_ev, d_e, d_v)]
    rec["d_ev_bytes_equal"] = bool(got["atomic"][1].tobytes() == got["ordered"][1].tobytes())
    for k, name in ((0, "f"), (2, "eatom"), (3, "vatom")):
        a, o = got["atomic"][k], got["ordered"][k]
        rec[f"max_difference_{name}_over_largest_entry"] = float(f"{np.abs(a - o).max() / np.abs(a).max():.3g}")
    rec["ms_ordered_ev_in_kernel"] = round(rec["ms_ordered_forces_ev"] - rec["ms_ordered_forces"], 4)
    per_step = (rec["ms_transpose_pair_list"] + rec["ms_transpose_fix_list"]) / 10.0
    rec["ms_transposes_per_step_at_one_reneighbouring_in_10"] = round(per_step, 4)
    for name in outputs:
        rec[f"ms_ordered_minus_atomic_per_step_{name}"] = round(
            rec[f"ms_ordered_{name}"] - rec[f"ms_atomic_{name}"] + rec["ms_gaussian_ordered"] - rec["ms_gaussian_atomic"] + per_step, 4)
    print(json.dumps(rec), flush=True)
    fx.close()


if __name__ == "__main__":
    main()
