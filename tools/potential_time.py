"""Cost of the exact Ewald per-atom potential (conp_ewald_compute, conp_ewald_compute_group_potential).

    python tools/potential_time.py [--reps N] [--warmup W] [--no-big]

Three cases: the headline box (4096 electrode + 32768 electrolyte, ffield) with all 36 864 atoms as targets, the same box with its
4096 electrode atoms as targets, and the 16384 / 262144 box (all atoms).  Per case: ms per conp_ewald_compute (the structure factor
of every charged atom), ms per conp_ewald_compute_group_potential right after it (the projection onto the targets: the group entry
reuses the cached structure factor) and their sum (what one `compute potential/atom` costs), after W warm-up calls as bench.py warms
up its update.  Prints one JSON line per case.  For the headline box with all atoms as targets the same process also times
conp_ewald_compute_forces for all atoms on the cached structure factor (forces, energy, virial) beside the
group potential: ms_forces in that case's line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lammps-user-conp2_amd"))


def box(name):
    from conp_amd import systems
    if name == "headline":     # bench.py --workload headline
        return systems.synthetic_fast(n_cells_x=32, n_cells_y=16, lz=600.0, n_elyte=32768, cutoff=16.0, accuracy_relative=1e-7,
                                      g_ewald=0.21218, mode="ffield", seed=12345)
    return systems.synthetic_fast(n_cells_x=64, n_cells_y=32, lz=1200.0, n_elyte=262144, cutoff=12.0, accuracy_relative=1e-6,
                                  g_ewald=0.2554, mode="ffield", seed=12345)         # bench.py --workload big


def measure(fx, at, sel, reps, warmup):
    for _ in range(warmup):
        fx.ewald_compute(at)
        fx.ewald_group_potential(at, sel)
    t_s = t_p = 0.0
    for _ in range(reps):
        t0 = time.perf_counter()
        fx.ewald_compute(at)
        t1 = time.perf_counter()
        fx.ewald_group_potential(at, sel)
        t2 = time.perf_counter()
        t_s += t1 - t0; t_p += t2 - t1
    return 1e3 * t_s / reps, 1e3 * t_p / reps


def measure_forces(fx, at, reps, warmup):
    """conp_ewald_compute_forces on the structure factor a conp_ewald_compute cached: the counterpart of the projection above"""
    f = np.zeros((at.nlocal, 3))
    fx.ewald_compute(at)
    for _ in range(warmup):
        fx.ewald_forces(at, f=f)
    t0 = time.perf_counter()
    for _ in range(reps):
        fx.ewald_forces(at, f=f)
    return 1e3 * (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-big", action="store_true")
    args = ap.parse_args()
    from conp_amd import FixConp, neighbor
    cases = [("headline", "all"), ("headline", "electrode")] + ([] if args.no_big else [("big", "all")])
    handles = {}
    for name, which in cases:
        if name not in handles:
            s = box(name)
            at, alist, blist = neighbor.build_lists(s)
            fx = FixConp(s)
            fx.init_lists(alist, blist)
            fx.setup_post_neighbor(at)                  # the k tables; the charges as the box has them
            handles[name] = (s, at, fx)
        s, at, fx = handles[name]
        n = at.nlocal
        sel = np.ones(n, np.int32) if which == "all" else (at.echeck[:n] != 0).astype(np.int32)
        t_s, t_p = measure(fx, at, sel, args.reps, args.warmup)
        info = fx.info()
        rec = dict(box=name, targets=which, n_targets=int(sel.sum()), n_atoms=int(n), kcount=int(info.kcount),
                   ms_ewald_compute=round(t_s, 4), ms_projection=round(t_p, 4), ms_total=round(t_s + t_p, 4), reps=args.reps, warmup=args.warmup)
        if (name, which) == ("headline", "all"):
            rec["ms_forces"] = round(measure_forces(fx, at, args.reps, args.warmup), 4)
        print(json.dumps(rec), flush=True)
    for s, at, fx in handles.values():
        fx.close()


if __name__ == "__main__":
    main()
