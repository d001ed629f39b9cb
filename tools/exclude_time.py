"""neigh_modify exclude in the device list build, and fix zmirror, on the headline box in one process.

    python tools/exclude_time.py [--reps N] [--warmup W]

The headline box of bench.py (4096 electrode + 32768 electrolyte atoms, ffield, cutoff 16 A, skin 2 A: cutneigh 18 A), newton off and
newton on (a handle each).  After W warm-up calls each, N calls of
  build            conp_pair_build_list_device; synchronous: wall time per call
  build_zero       conp_pair_build_list_exclude_device with no rule in force (the plain build by contract)
  build_group      the same with one group rule: the upper-z half of the electrolyte excluded among itself (the shape of the zmirror
                   deck's `neigh_modify exclude group solpos solpos`), with its pair count
  build_all_kinds  one type pair, one group pair, molecule/intra and molecule/inter at once (molecule = (tag - 1) // 4 + 1)
  pair             conp_pair_compute_device (forces and the eight sums) on the plain list and on the group-rule list: N calls
                   enqueued back to back, one synchronisation behind the last
  mirror           conp_zmirror_post_integrate_device, lower-z half of the electrolyte onto the upper-z half by tag order: N calls
                   enqueued back to back, one synchronisation behind the last
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

UPPER, LOWER = 2, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("exclude_time.py: no GPU")
    torch.cuda.init()
    from conp_amd import FixConp, neighbor
    from neigh_time import timed
    from pair_time import lj_tables
    from pppm_force_time import box
    s0, _mesh, _order = box("headline")
    s0 = dataclasses.replace(s0, eletypes=None)
    at = neighbor.make_ghosts(s0)
    n, nall, cutneigh = at.nlocal, at.nall, float(s0.cutoff + s0.skin)
    # the electrolyte split in two halves of equal size by z; a tag order in which the k-th atom of the lower half mirrors onto the
    # k-th of the upper half (what the mirror needs is the map, not a physical mirror image)
    el = np.nonzero(at.echeck[:n] == 0)[0]
    el = el[np.argsort(at.x[el, 2], kind="stable")]
    half = len(el) // 2
    mask = np.ones(n, np.int32)
    mask[el[:half]] |= LOWER
    mask[el[half:2 * half]] |= UPPER
    mtag = np.arange(2 * half + 1, 2 * half + 1 + n, dtype=np.int32)             # the others: tags behind the two ranges
    mtag[el[:half]] = np.arange(1, half + 1)
    mtag[el[half:2 * half]] = np.arange(half + 1, 2 * half + 1)
    own = np.asarray(at.owner, dtype=np.int64)
    molecule = ((at.tag.astype(np.int64) - 1) // 4 + 1).astype(np.int32)
    dev = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).cuda()
    d_x, d_q = dev(at.x, np.float64), dev(at.q, np.float64)
    d_type, d_mask, d_mol = dev(at.type, np.int32), dev(mask[own], np.int32), dev(molecule, np.int32)
    d_f = torch.zeros((nall, 3), dtype=torch.float64, device="cuda")
    d_ev = torch.zeros(8, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    sync = torch.cuda.synchronize
    rec = dict(box="headline", n_owned=int(n), n_all=int(nall), cutneigh=cutneigh, reps=args.reps, warmup=args.warmup,
               upper_half_atoms=int(half))
    for newton in (False, True):
        tag = "newton_on" if newton else "newton_off"
        s = dataclasses.replace(s0, newton=newton)
        fx = FixConp(s)
        fx.pair_set_params(s.cutsq_table(), s.cutoff, lj_tables(s.ntypes, s.cutoff))
        lst = neighbor.NeighList(inum=0, ilist=np.zeros(0, np.int32), numneigh=np.zeros(nall, np.int32), first=np.zeros(nall, np.int32),
                                 neigh=np.zeros(0, np.int32))
        fx.init_lists(lst, lst)
        fx.setup_post_neighbor(at)                                               # the type array conp_pair_compute_device reads
        plain = lambda: fx.pair_build_list_device(d_x.data_ptr(), n, nall, cutneigh)
        excl = lambda: fx.pair_build_list_exclude_device(d_x.data_ptr(), n, nall, cutneigh, d_type.data_ptr(), d_mask.data_ptr(),
                                                         d_mol.data_ptr())
        pair = lambda: fx.pair_compute_device(d_x.data_ptr(), d_q.data_ptr(), d_f.data_ptr(), d_ev.data_ptr(), 0, 0)
        t = lambda fn: round(timed(fn, args.reps, args.warmup, sync), 4)
        rec[f"ms_build_{tag}"] = t(plain)
        rec[f"pairs_{tag}"] = int(fx.pair_get_list()[0].neigh.size)
        rec[f"ms_pair_{tag}"] = t(pair)
        fx.pair_set_exclusions()
        rec[f"ms_build_zero_{tag}"] = t(excl)
        fx.pair_set_exclusions(s.ntypes, type_pairs=[(1, 2)], group_pairs=[(UPPER, UPPER)], molecule=[(1, 1), (UPPER, 0)])
        rec[f"ms_build_all_kinds_{tag}"] = t(excl)
        rec[f"pairs_all_kinds_{tag}"] = int(fx.pair_get_list()[0].neigh.size)
        fx.pair_set_exclusions(group_pairs=[(UPPER, UPPER)])
        rec[f"ms_build_group_{tag}"] = t(excl)
        rec[f"pairs_group_{tag}"] = int(fx.pair_get_list()[0].neigh.size)
        rec[f"ms_pair_group_{tag}"] = t(pair)
        if not newton:
            fx.zmirror_set_params(mtag, mask, LOWER, UPPER, 1, float(s.boxlo[2]), float(s.prd[2]))
            d_xm = d_x.clone()
            rec["mirror_pairs"] = int(len(fx.zmirror_get_map()[0]))
            rec["ms_mirror"] = round(timed(lambda: fx.zmirror_post_integrate_device(d_xm.data_ptr(), 0), args.reps, args.warmup, sync), 5)
        fx.close()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
