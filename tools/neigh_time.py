"""The pair style's half list at a re-neighbouring step: built on the device from d_x, against the upload it replaces, in one process
(DESIGN.md section 17).

    python tools/neigh_time.py [--reps N] [--warmup W]

The headline box of bench.py (4096 electrode + 32768 electrolyte atoms, ffield, cutoff 16 A, skin 2 A: cutneigh 18 A).  After W warm-up
calls each, N calls of
  build          conp_pair_build_list_device, newton off and newton on (a handle each); synchronous: wall time per call
  build_special  the same with a special-bond table: the electrolyte atoms chained by tag (1-2, 1-3, 1-4 partners), prd_half of the box
  set_list       conp_pair_set_list of the IDENTICAL list (the one the build produced, downloaded once): the host-side index check
                 and the upload a device-resident engine no longer needs.  Building that list on the host, and copying x back to do
                 so, are NOT in this number
  moved          conp_pair_list_moved_device: N calls enqueued back to back, one synchronisation behind the last
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


def chain_tables(at, maxspecial=6):
    """nspecial [nlocal][3] (cumulative), special [nlocal][maxspecial]: the owned electrolyte atoms chained in tag order"""
    n = at.nlocal
    el = np.nonzero(at.echeck[:n] == 0)[0]
    el = el[np.argsort(at.tag[el], kind="stable")]
    m = len(el)
    nspecial, special = np.zeros((n, 3), np.int32), np.zeros((n, maxspecial), np.int32)
    fill = np.zeros(n, np.int64)
    for c, d in enumerate((1, 2, 3)):
        for sgn in (-1, 1):
            k = np.arange(m)
            ok = (k + sgn * d >= 0) & (k + sgn * d < m)
            i, j = el[k[ok]], el[k[ok] + sgn * d]
            special[i, fill[i]] = at.tag[j]
            fill[i] += 1
        nspecial[:, c] = fill
    return nspecial, special


def timed(fn, reps, warmup, sync):
    for _ in range(warmup):
        fn()
    sync()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    sync()
    return 1e3 * (time.perf_counter() - t0) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("neigh_time.py: no GPU")
    torch.cuda.init()
    from conp_amd import FixConp, neighbor
    from pair_time import lj_tables
    from pppm_force_time import box
    s0, _mesh, _order = box("headline")
    s0 = dataclasses.replace(s0, eletypes=None)
    at = neighbor.make_ghosts(s0)
    nall, cutneigh = at.nall, float(s0.cutoff + s0.skin)
    prd_half = [0.5 * float(p) if per else 0.0 for p, per in zip(s0.prd, s0.periodic)]
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).cuda()
    d_x = dev(at.x, np.float64)
    nsp, sp = chain_tables(at)
    d_tag, d_nsp, d_sp = dev(at.tag, np.int32), dev(nsp, np.int32), dev(sp, np.int32)
    d_flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    rec = dict(box="headline", n_owned=int(at.nlocal), n_all=int(nall), cutneigh=cutneigh, reps=args.reps, warmup=args.warmup)
    for newton in (False, True):
        tag = "newton_on" if newton else "newton_off"
        s = dataclasses.replace(s0, newton=newton)
        fx = FixConp(s)
        fx.pair_set_params(s.cutsq_table(), s.cutoff, lj_tables(s.ntypes, s.cutoff), (1.0, 0.0, 0.0, 0.5), (1.0, 0.0, 0.0, 0.8333))
        plain = lambda: fx.pair_build_list_device(d_x.data_ptr(), at.nlocal, nall, cutneigh)
        special = lambda: fx.pair_build_list_device(d_x.data_ptr(), at.nlocal, nall, cutneigh, d_tag.data_ptr(), d_nsp.data_ptr(),
                                                    d_sp.data_ptr(), sp.shape[1], prd_half)
        rec[f"ms_build_special_{tag}"] = round(timed(special, args.reps, args.warmup, torch.cuda.synchronize), 4)
        rec[f"ms_build_{tag}"] = round(timed(plain, args.reps, args.warmup, torch.cuda.synchronize), 4)
        lst, _ = fx.pair_get_list()
        rec[f"listed_pairs_{tag}"] = int(lst.neigh.size)
        rec[f"ms_moved_{tag}"] = round(timed(lambda: fx.pair_list_moved_device(d_x.data_ptr(), 0.5 * s.skin, d_flag.data_ptr()),
                                             args.reps, args.warmup, torch.cuda.synchronize), 4)
        rec[f"ms_set_list_{tag}"] = round(timed(lambda: fx.pair_set_list(lst, nall), args.reps, args.warmup, torch.cuda.synchronize), 4)
        rec[f"list_megabytes_{tag}"] = round(4e-6 * (lst.neigh.size + 2 * nall + lst.inum), 2)
        fx.close()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
