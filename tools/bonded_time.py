"""The harmonic bond and angle forces of a step from device arrays, beside the pair entry's time in the same process (DESIGN.md
section 21).

    python tools/bonded_time.py [--reps N] [--warmup W]

The headline box of bench.py (4096 electrode + 32768 electrolyte atoms, ffield).  The 32768 electrolyte atoms are grouped three at a
time into molecules (10922 molecules: 2 bonds and 1 angle each; owned indices and the box lengths, the closest-image form); the
outer atoms of a molecule are placed 1 A from its middle atom at 104.5 degrees, so that the terms are of a deck's size.  After W
warm-up calls each, N calls of conp_bonded_compute_device enqueued back to back with ONE synchronisation behind the last
(wall = (enqueue + the final wait) / N, host = the enqueue loop alone / N), split by outputs: forces only; forces and d_ev; forces,
d_ev, eatom and vatom -- and the same for conp_pair_compute_device over the pair style's half list of the same atoms, and for the
host entry conp_bonded_compute (the route the device entry removes: coordinates up, forces down).  Prints one JSON line.
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


def molecules(s, seed=3):
    """-> (x with the outer atoms of every molecule placed around its middle atom and wrapped, bonds, angles)"""
    el = np.nonzero(s.echeck == 0)[0]
    mol = el[:len(el) // 3 * 3].reshape(-1, 3)
    n = len(mol)
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3)); u /= np.linalg.norm(u, axis=1)[:, None]
    w = np.cross(u, rng.normal(size=(n, 3))); w /= np.linalg.norm(w, axis=1)[:, None]
    th = np.deg2rad(104.5)
    x = s.x.copy()
    x[mol[:, 0]] = x[mol[:, 1]] + u
    x[mol[:, 2]] = x[mol[:, 1]] + np.cos(th) * u + np.sin(th) * w
    for c in range(3):
        if s.periodic[c]:
            x[:, c] = np.where(x[:, c] < s.boxlo[c], x[:, c] + s.prd[c], x[:, c])
            x[:, c] = np.where(x[:, c] >= s.boxhi[c], x[:, c] - s.prd[c], x[:, c])
    one = np.ones(n, dtype=np.int32)
    bonds = np.stack([np.stack([mol[:, 1], mol[:, 0], one], 1), np.stack([mol[:, 1], mol[:, 2], one], 1)], 1).reshape(-1, 3)
    angles = np.stack([mol[:, 0], mol[:, 1], mol[:, 2], one], 1)
    return np.ascontiguousarray(x), bonds, angles


def timed(call, reps, warmup, sync):
    for _ in range(warmup):
        call()
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        call()
    t1 = time.perf_counter()
    sync()
    t2 = time.perf_counter()
    return round(1e3 * (t2 - t0) / reps, 4), round(1e3 * (t1 - t0) / reps, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bonded_time.py: no GPU")
    torch.cuda.init()
    from conp_amd import FixConp, neighbor
    from pair_time import lj_tables
    from pppm_force_time import box, charge_electrodes
    s, _mesh, _order = box("headline")
    at, alist, blist = neighbor.build_lists(s)
    charge_electrodes(at)
    pairs = neighbor.build_lists(dataclasses.replace(s, eletypes=None))[1]       # the pair style's list: every pair
    nall, n = at.nall, at.nlocal
    fx = FixConp(s)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.pair_set_params(s.cutsq_table(), s.cutoff, lj_tables(s.ntypes, s.cutoff))
    fx.pair_set_list(pairs, nall)
    xm, bonds, angles = molecules(s)
    xb = at.x.copy(); xb[:n] = xm                                                # (ghost rows are not read: owned indices)
    fx.bonded_set_params([450.0], [1.0], [55.0], [np.deg2rad(104.52)], newton_bond=True)
    fx.bonded_set_lists(n, nall, bonds, angles, np.where(s.periodic, s.prd, 0.0))
    atb = dataclasses.replace(at, x=np.ascontiguousarray(xb))
    f = np.zeros((nall, 3))
    d_x = torch.from_numpy(np.ascontiguousarray(at.x)).cuda()
    d_xb = torch.from_numpy(atb.x).cuda()
    d_q = torch.from_numpy(at.q.copy()).cuda()
    d_f = torch.zeros((nall, 3), dtype=torch.float64, device="cuda")
    d_ev = torch.zeros(8, dtype=torch.float64, device="cuda")
    d_e = torch.zeros(nall, dtype=torch.float64, device="cuda")
    d_v = torch.zeros((nall, 6), dtype=torch.float64, device="cuda")
    outputs = {"forces": (False, False), "forces_ev": (True, False), "forces_ev_atom": (True, True)}
    rec = dict(box="headline", n_owned=int(n), n_all=int(nall), molecules=len(angles), bonds=len(bonds), angles=len(angles),
               listed_pairs=int(pairs.npairs), reps=args.reps, warmup=args.warmup)
    for name, (ev, atom) in outputs.items():
        def bonded():
            fx.bonded_compute_device(d_xb.data_ptr(), d_f.data_ptr(), d_ev.data_ptr() if ev else 0, d_e.data_ptr() if atom else 0,
                                     d_v.data_ptr() if atom else 0)

        def pair():
            fx.pair_compute_device(d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), d_ev.data_ptr() if ev else 0,
                                   d_e.data_ptr() if atom else 0, d_v.data_ptr() if atom else 0)

        def host():
            fx.bonded_compute(atb, f=f, eng=ev, virial=ev, eatom=atom, vatom=atom)
        rec[f"ms_bonded_device_{name}_wall"], rec[f"ms_bonded_device_{name}_host_thread"] = timed(bonded, args.reps, args.warmup, torch.cuda.synchronize)
        rec[f"ms_pair_device_{name}_wall"], _ = timed(pair, max(args.reps // 10, 5), 3, torch.cuda.synchronize)
        rec[f"ms_bonded_host_{name}"], _ = timed(host, max(args.reps // 10, 5), 3, lambda: None)
    print(json.dumps(rec), flush=True)
    fx.close()


if __name__ == "__main__":
    main()
