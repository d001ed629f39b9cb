"""The real-space pair forces (lj/cut/coul/long) of a step from host arrays and from device arrays, in one process (DESIGN.md
section 16).

    python tools/pair_time.py [--reps N] [--warmup W]

The headline box of bench.py (4096 electrode + 32768 electrolyte atoms, ffield, the box's own cutoff of 16 A, skin 2 A), the pair
style's generic half list over all atoms, synthetic LJ coefficients (epsilon 0.05-0.4, sigma 2.5-3.5, arithmetic mixing, shifted).
After W warm-up calls each, N calls of
  host entry     conp_pair_compute (host arrays in and out; synchronous: wall time per call)
  device entry   conp_pair_compute_device on device copies of the same atoms: N calls enqueued back to back, ONE synchronisation
                 behind the last; wall = (enqueue + the final wait) / N, host = the enqueue loop alone / N
each split by outputs: forces only; forces, energy and virial; forces, energy, virial, eatom and vatom.  Prints one JSON line with the
times, the number of listed pairs and the listed pairs per second of the device entry, and beside them the 2.72 / 0.78 ms of the
k-space device entries on the same box (Ewald / PPPM), so that a reader sees which half of the step dominates.
Needs a GPU: there is no fall-back."""
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


def lj_tables(ntypes, cutoff, seed=3):
    n = ntypes + 1
    rng = np.random.default_rng(seed)
    eps, sig = rng.uniform(0.05, 0.4, n), rng.uniform(2.5, 3.5, n)
    e, s = np.sqrt(eps[:, None] * eps[None, :]), 0.5 * (sig[:, None] + sig[None, :])
    cut = np.full((n, n), float(cutoff))
    return dict(cut_ljsq=cut * cut, lj1=48 * e * s ** 12, lj2=24 * e * s ** 6, lj3=4 * e * s ** 12, lj4=4 * e * s ** 6,
                offset=4 * e * ((s / cut) ** 12 - (s / cut) ** 6))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("pair_time.py: no GPU")
    torch.cuda.init()
    from conp_amd import FixConp, neighbor
    from pppm_force_time import box, charge_electrodes
    s, _mesh, _order = box("headline")
    at, alist, blist = neighbor.build_lists(s)
    charge_electrodes(at)
    pairs = neighbor.build_lists(dataclasses.replace(s, eletypes=None))[1]       # the pair style's list: every pair
    nall = at.nall
    fx = FixConp(s)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.pair_set_params(s.cutsq_table(), s.cutoff, lj_tables(s.ntypes, s.cutoff))
    fx.pair_set_list(pairs, nall)
    f = np.zeros((nall, 3))
    d_x = torch.from_numpy(np.ascontiguousarray(at.x)).cuda()
    d_q = torch.from_numpy(at.q.copy()).cuda()
    d_f = torch.zeros((nall, 3), dtype=torch.float64, device="cuda")
    d_ev = torch.zeros(8, dtype=torch.float64, device="cuda")
    d_e = torch.zeros(nall, dtype=torch.float64, device="cuda")
    d_v = torch.zeros((nall, 6), dtype=torch.float64, device="cuda")
    outputs = {"forces": (False, False), "forces_ev": (True, False), "forces_ev_atom": (True, True)}
    rec = dict(box="headline", n_owned=int(at.nlocal), n_all=int(nall), cutoff=float(s.cutoff), listed_pairs=int(pairs.npairs),
               reps=args.reps, warmup=args.warmup, ms_kspace_device_ewald=2.72, ms_kspace_device_pppm=0.78)
    for name, (ev, atom) in outputs.items():
        def host():
            fx.pair_compute(at, f=f, eng=ev, virial=ev, eatom=atom, vatom=atom)

        def device():
            fx.pair_compute_device(d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), d_ev.data_ptr() if ev else 0,
                                   d_e.data_ptr() if atom else 0, d_v.data_ptr() if atom else 0)
        for _ in range(args.warmup):
            host()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            host()
        ms_host = 1e3 * (time.perf_counter() - t0) / args.reps
        for _ in range(args.warmup):
            device()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            device()
        t1 = time.perf_counter()
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        wall = 1e3 * (t2 - t0) / args.reps
        rec[f"ms_host_{name}"] = round(ms_host, 4)
        rec[f"ms_device_{name}_wall"] = round(wall, 4)
        rec[f"ms_device_{name}_host_thread"] = round(1e3 * (t1 - t0) / args.reps, 4)
        rec[f"listed_pairs_per_s_device_{name}"] = float(f"{pairs.npairs / (wall * 1e-3):.4g}")
    print(json.dumps(rec), flush=True)
    fx.close()


if __name__ == "__main__":
    main()
