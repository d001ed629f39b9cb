"""Cost of the PPPM reciprocal-space forces on the device (conp_pppm_compute_forces) beside the exact sum.

    python tools/pppm_force_time.py [--reps N] [--warmup W] [--no-big]

Three boxes: il_onelayer on 40 x 45 x 180 (order 5), the headline box (4096 electrode + 32768 electrolyte, ffield) and the
16384 / 262144 box.  The meshes of the two large boxes are chosen for about the RMS force accuracy of the handle's Ewald `accuracy`
(DESIGN.md section 13 says how).  Per box, after W warm-up calls: wall ms per conp_pppm_compute_forces (forces, energy, virial of all
atoms, host arrays in and out), then the same calls once more with an event pair around each phase (conp_fix_profile): spread,
forward transform, k-space kernel, backward transforms, gather, in ms of device time.  For comparison, in the same process and on the
same box: ms per conp_ewald_compute + conp_ewald_compute_forces on an Ewald handle (the structure factor of the atoms given, then
forces, energy, virial).  Prints one JSON line per box."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lammps-user-conp2_amd"))

PHASES = ("pppm_f_spread", "pppm_f_forward", "pppm_f_kspace", "pppm_f_backward", "pppm_f_gather")


def box(name):
    from conp_amd import systems
    if name == "il_onelayer":
        return systems.deck("il_onelayer", "ffield", etypes=True), (40, 45, 180), 5
    if name == "headline":     # bench.py --workload headline
        return systems.synthetic_fast(n_cells_x=32, n_cells_y=16, lz=600.0, n_elyte=32768, cutoff=16.0, accuracy_relative=1e-7,
                                      g_ewald=0.21218, mode="ffield", seed=12345), (72, 64, 540), 5
    return systems.synthetic_fast(n_cells_x=64, n_cells_y=32, lz=1200.0, n_elyte=262144, cutoff=12.0, accuracy_relative=1e-6,
                                  g_ewald=0.2554, mode="ffield", seed=12345), (180, 150, 1296), 5         # bench.py --workload big


def charge_electrodes(at, seed=11):
    """seeded electrode charges (a solve is not what is timed)"""
    n = at.nlocal
    ele = at.echeck[:n] != 0
    at.q[:n][ele] = np.random.default_rng(seed).uniform(0.005, 0.02, int(ele.sum())) * at.echeck[:n][ele]
    at.q[n:] = at.q[at.owner[n:]]


def wall(call, reps, warmup):
    for _ in range(warmup):
        call()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    return 1e3 * (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--no-big", action="store_true")
    args = ap.parse_args()
    from conp_amd import FixConp, neighbor
    for name in ["il_onelayer", "headline"] + ([] if args.no_big else ["big"]):
        s, mesh, order = box(name)
        at, alist, blist = neighbor.build_lists(s)
        charge_electrodes(at)
        n = at.nlocal
        f = np.zeros((n, 3))
        fp = FixConp(s, extra_args=["pppm"], pppm_mesh=mesh, pppm_order=order)
        fp.init_lists(alist, blist)
        fp.setup_post_neighbor(at)
        ms_pppm = wall(lambda: fp.pppm_compute_forces(at, f=f), args.reps, args.warmup)
        fp.profile(1)
        for _ in range(args.reps):
            fp.pppm_compute_forces(at, f=f)
        prof = fp.profile_read()
        fp.profile(0)
        fp.close()
        fe = FixConp(s)
        fe.init_lists(alist, blist)
        fe.setup_post_neighbor(at)

        def exact():
            fe.ewald_compute(at)
            fe.ewald_forces(at, f=f)
        ms_ewald = wall(exact, args.reps, args.warmup)
        kcount = int(fe.info().kcount)
        fe.close()
        rec = dict(box=name, n_atoms=int(n), mesh=list(mesh), order=order, kcount=kcount, ms_pppm_forces=round(ms_pppm, 4),
                   ms_ewald_compute_plus_forces=round(ms_ewald, 4), ratio=round(ms_ewald / ms_pppm, 3), reps=args.reps, warmup=args.warmup)
        for ph in PHASES:
            rec["ms_" + ph[len("pppm_f_"):]] = round(prof[ph][0], 4) if ph in prof else None
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
