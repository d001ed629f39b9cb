"""conp_potential_atom_device beside the host entry conp_compute_potential_atom, in one process.

    python tools/potential_device_time.py [--reps N] [--warmup W]

The headline box of tools/ordered_pair_time.py and its method for the device entry: after W warm-up calls, N calls enqueued back to
back and ONE synchronisation behind the last; wall = (enqueue + the final wait) / N.  The host entry synchronises itself: wall time
per call.  Three selections -- the electrode atoms (4096 at the headline size), 4 zero-charge probes, every owned atom -- each
  host          conp_compute_potential_atom (uploads x, q and the list, float64 atomics, host tail)
  device        conp_potential_atom_device, reuse_kspace = 0 (its own structure factor)
  device_reuse  conp_potential_atom_device, reuse_kspace = 1 behind one conp_ewald_compute_forces_device
  pair_only     conp_potential_atom_device, pair part alone
with the eta correction on the electrode molecules, and the largest difference of the device entry from the host entry on the
selected owned rows.  There is no target time: the comparison is the host entry in the same process.  Prints one JSON line.  Needs a
GPU: there is no fall-back."""
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
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("potential_device_time.py: no GPU")
    torch.cuda.init()
    from conp_amd import FixConp, capi, neighbor
    from pppm_force_time import box, charge_electrodes
    s, _mesh, _order = box("headline")
    el = np.nonzero((s.echeck == 0) & (s.q != 0))[0][:4]
    q, x = s.q.copy(), s.x.copy()
    centre = s.boxlo + 0.5 * np.asarray(s.prd)
    for k, i in enumerate(el):                                       # four zero-charge probes at the box centre
        q[i] = 0.0
        x[i] = centre + np.array([0.37 * k, -0.21 * k, 0.53 * k - 0.8])
    s = dataclasses.replace(s, x=x, q=q)
    at, alist, blist = neighbor.build_lists(s)
    charge_electrodes(at)
    n, nall = at.nlocal, at.nall
    pairs = neighbor.build_lists(dataclasses.replace(s, eletypes=None))[1]       # the pair style's list: every pair
    fx = FixConp(s)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)
    fx.pair_set_list(pairs, nall)
    fx.pair_transpose_list_device()
    d_x = torch.from_numpy(np.ascontiguousarray(at.x)).cuda()
    d_q = torch.from_numpy(at.q.copy()).cuda()
    d_f = torch.zeros((nall, 3), dtype=torch.float64, device="cuda")
    d_pot = torch.zeros(nall, dtype=torch.float64, device="cuda")
    X, Q = d_x.data_ptr(), d_q.data_ptr()
    etasel = (at.echeck != 0).astype(np.int32)
    ele, probe = (at.echeck != 0).astype(np.int32), np.zeros(nall, np.int32)
    probe[el] = 1
    probe[n:] = probe[at.owner[n:]]
    rec = dict(box="headline", n_owned=int(n), n_all=int(nall), listed_pairs=int(pairs.npairs), reps=args.reps, warmup=args.warmup,
               eta=float(s.eta), list_bytes_uploaded_by_the_host_entry=int(4 * (pairs.npairs + 2 * nall + pairs.inum)))

    def stream_timed(call, key):
        for _ in range(args.warmup):
            call()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.reps):
            call()
        torch.cuda.synchronize()
        rec[key] = round(1e3 * (time.perf_counter() - t0) / args.reps, 4)

    stream_timed(lambda: fx.ewald_forces_device(X, Q, d_f.data_ptr(), 0, 0), "ms_ewald_forces_device")
    for name, sel in (("electrodes", ele), ("probes", probe), ("all", np.ones(nall, np.int32))):
        flags, targets, nt = capi.potential_selection(sel, etasel, n)
        F, T = torch.from_numpy(flags).cuda(), torch.from_numpy(targets).cuda()
        torch.cuda.synchronize()
        rec[f"ntargets_{name}"] = nt
        dev = lambda **kw: fx.potential_atom_device(X, Q, F.data_ptr(), nt, T.data_ptr(), d_pot.data_ptr(), eta=s.eta, **kw)
        stream_timed(lambda: fx.compute_potential_atom(at, pairs, sel, etasel, eta=s.eta), f"ms_host_{name}")
        stream_timed(lambda: dev(), f"ms_device_{name}")
        fx.ewald_forces_device(X, Q, d_f.data_ptr(), 0, 0)
        stream_timed(lambda: dev(reuse_kspace=True), f"ms_device_reuse_{name}")
        stream_timed(lambda: dev(kspace=False), f"ms_pair_only_{name}")
        # faster and different is not faster: both entries once more, at the size that was timed
        want = fx.compute_potential_atom(at, pairs, sel, etasel, eta=s.eta)
        fx.ewald_forces_device(X, Q, d_f.data_ptr(), 0, 0)
        dev(reuse_kspace=True)
        torch.cuda.synchronize()
        got = d_pot.cpu().numpy()
        own = np.nonzero(sel[:n])[0]
        if s.newton:
            got, want = got.copy(), want.copy()
            np.add.at(got, at.owner[n:], got[n:]); np.add.at(want, at.owner[n:], want[n:])
        rec[f"max_difference_over_largest_entry_{name}"] = float(f"{np.abs(got[own] - want[own]).max() / np.abs(want[own]).max():.3g}")
    print(json.dumps(rec), flush=True)
    fx.close()


if __name__ == "__main__":
    main()
