"""The fix's re-neighbouring step: conp_fix_post_neighbor_device against the host route it replaces, for the identical list, in one
process.

    python tools/post_neighbor_time.py [--reps N] [--warmup W]

The headline box of bench.py (4096 electrode + 32768 electrolyte atoms, ffield, cutoff 16 A, skin 2 A).  One handle, set up once with
host arrays; its ghosts and its half list are built on the device.  After W warm-up calls each, N calls of
  device      conp_fix_post_neighbor_device; synchronous: wall time per call, its synchronisations included
  host_route  what a device-resident engine did before: conp_pair_get_list + conp_ghost_get + x and q copied to the host (pageable
              memory, as LAMMPS' arrays are) + conp_fix_init_list + conp_fix_post_neighbor, which uploads the same list again
  host_hook   conp_fix_post_neighbor alone on arrays that are already on the host (the hook's own cost, without the round trip)
Prints one JSON line.  Needs a GPU: there is no fall-back."""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lammps-user-conp2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("post_neighbor_time.py: no GPU")
    torch.cuda.init()
    from conp_amd import FixConp, neighbor
    from neigh_time import timed
    from pppm_force_time import box
    s, _mesh, _order = box("headline")
    s = dataclasses.replace(s, eletypes=None)
    at = neighbor.make_ghosts(s)
    n, nall, cut = at.nlocal, at.nall, float(s.cutoff + s.skin)
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).cuda()
    d_x, d_q = dev(at.x, np.float64), dev(at.q, np.float64)
    sync = torch.cuda.synchronize
    sync()
    fx = FixConp(s)
    fx.pair_set_params(s.cutsq_table(), s.cutoff)
    nghost = fx.ghost_build_device(d_x.data_ptr(), n, s.boxlo, s.boxhi, s.periodic, cut)
    if n + nghost != nall:
        raise SystemExit(f"post_neighbor_time.py: {nghost} ghosts, make_ghosts has {at.nghost}")
    fx.ghost_fill_device(d_x.data_ptr(), d_q.data_ptr())
    fx.pair_build_list_device(d_x.data_ptr(), n, nall, cut)
    lst, _ = fx.pair_get_list()
    fx.init_lists(lst, lst)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)
    rec = dict(box="headline", n_owned=int(n), n_ghost=int(nghost), listed_pairs=int(lst.neigh.size),
               list_megabytes=round(4e-6 * (lst.neigh.size + 2 * nall + lst.inum), 2), reps=args.reps, warmup=args.warmup,
               arch=torch.cuda.get_device_properties(0).gcnArchName.split(":")[0])
    rec["ms_device"] = round(timed(lambda: fx.post_neighbor_device(d_x.data_ptr(), d_q.data_ptr()), args.reps, args.warmup, sync), 4)
    rec["zn_cols_device"] = int(fx.info().zn_cols)
    h_x, h_q = torch.empty((nall, 3), dtype=torch.float64), torch.empty((nall,), dtype=torch.float64)
    full = np.concatenate([np.arange(n), at.owner[n:]])

    def host_route():
        got, _ = fx.pair_get_list()
        _, _, owner, _ = fx.ghost_get()
        h_x.copy_(d_x)
        h_q.copy_(d_q)
        a = neighbor.Atoms(nlocal=n, nghost=len(owner), x=h_x.numpy(), q=h_q.numpy(), type=at.type, tag=at.tag, echeck=at.echeck, owner=full)
        fx.init_list(2, got)
        fx.post_neighbor(a)
    rec["ms_host_route"] = round(timed(host_route, args.reps, args.warmup, sync), 4)
    rec["zn_cols_host"] = int(fx.info().zn_cols)
    rec["ms_host_hook"] = round(timed(lambda: fx.post_neighbor(at), args.reps, args.warmup, sync), 4)
    fx.close()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
