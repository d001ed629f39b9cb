"""Ghost atoms kept on the device: the build at a re-neighbouring step and the per-step fill, fold and remap, against the copies the
host route needs, in one process.

    python tools/ghost_time.py [--reps N] [--warmup W]

The headline box of bench.py (4096 electrode + 32768 electrolyte atoms, ffield, cutoff 16 A, skin 2 A: cutghost 18 A).  After W warm-up
calls each, N calls of
  build        conp_ghost_build_device; synchronous: wall time per call, its synchronisations included
  fill         conp_ghost_fill_device (x and q)                     } N calls enqueued back to back,
  fold3        conp_ghost_fold_device at width 3 (forces)           } one synchronisation behind the last
  wrap         conp_atoms_wrap_device with image counters           }
  host_copies  what the host route moves per re-neighbour: the owned x to the host, the nall rows of x and q back (pageable memory,
               as LAMMPS' arrays are).  A floor: the host's own ghost construction is NOT in this number
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
        raise SystemExit("ghost_time.py: no GPU")
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
    d_f = torch.zeros((nall, 3), dtype=torch.float64, device="cuda")
    d_image = torch.zeros((n, 3), dtype=torch.int32, device="cuda")
    sync = torch.cuda.synchronize
    sync()
    fx = FixConp(s)
    build = lambda: fx.ghost_build_device(d_x.data_ptr(), n, s.boxlo, s.boxhi, s.periodic, cut)
    nghost = build()
    if n + nghost != nall:
        raise SystemExit(f"ghost_time.py: {nghost} ghosts, make_ghosts has {at.nghost}")
    rec = dict(box="headline", n_owned=int(n), n_ghost=int(nghost), cutghost=cut, reps=args.reps, warmup=args.warmup,
               arch=torch.cuda.get_device_properties(0).gcnArchName.split(":")[0])
    rec["ms_build"] = round(timed(build, args.reps, args.warmup, sync), 4)
    rec["ms_fill"] = round(timed(lambda: fx.ghost_fill_device(d_x.data_ptr(), d_q.data_ptr()), args.reps, args.warmup, sync), 4)
    rec["ms_fold3"] = round(timed(lambda: fx.ghost_fold_device(d_f.data_ptr(), 3), args.reps, args.warmup, sync), 4)
    rec["ms_wrap"] = round(timed(lambda: fx.atoms_wrap_device(d_x.data_ptr(), n, s.boxlo, s.boxhi, s.periodic, d_image.data_ptr()),
                                 args.reps, args.warmup, sync), 4)
    h_own, h_x, h_q = torch.empty((n, 3), dtype=torch.float64), torch.from_numpy(at.x.copy()), torch.from_numpy(at.q.copy())

    def host_copies():
        h_own.copy_(d_x[:n])
        d_x.copy_(h_x)
        d_q.copy_(h_q)
    rec["ms_host_copies"] = round(timed(host_copies, args.reps, args.warmup, sync), 4)
    fx.close()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
