"""`fix efield` from device arrays, beside the route an engine has without the entry.

    python tools/efield_time.py [--reps N] [--warmup W] [--no-coupled]

The headline box of bench.py (4096 electrode + 32768 electrolyte atoms, all 36864 owned atoms in the field's group), a field along z
of -1 V over the box length, image counters in -2 .. 2.  After W warm-up calls each, N calls enqueued back to back with ONE
synchronisation behind the last (wall = (enqueue + the final wait) / N, host = the enqueue loop alone / N); then 50 calls with an
event pair around each (conp_fix_profile: device = the time between the events, launches of one call included):
  - conp_efield_post_force_device for every output combination: forces alone (one launch), with d_out (two), with d_vatom, with both;
    and without image counters;
  - for scale conp_pair_compute_device (forces only) and conp_integrate_final_device on the same atoms;
  - the host route the entry replaces: x, q and f down, q E in numpy, f up;
  - coupled (a conq handle set up on the same box): conp_fix_pre_force_device followed by the coupled call, beside the same update
    followed by conp_fix_compute_scalar, a host-side field and the uncoupled call -- the round trip the coupled form removes.
d_f grows by q E per call: the field is small, and nothing reads the forces.
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

QE2F = 23.060549
FTM2V = 1.0 / 48.88821291 / 48.88821291
MVV2E = 48.88821291 * 48.88821291
BOLTZ = 0.0019872067
MASS = np.array([67.07, 15.04, 57.12, 144.96, 12.001])


def device_ms(fx, label, call, sync, reps=50):
    """per call, between the events conp_fix_profile puts around the entry's launches"""
    sync()
    fx.profile(1)
    for _ in range(reps):
        call()
    sync()
    ms, cnt = fx.profile_read().get(label, (0.0, 0))
    fx.profile(0)
    return round(ms, 5) if cnt else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--no-coupled", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("efield_time.py: no GPU")
    torch.cuda.init()
    from conp_amd import FixConp, neighbor
    from bonded_time import timed
    from pair_time import lj_tables
    from pppm_force_time import box, charge_electrodes
    s, _mesh, _order = box("headline")
    at, alist, blist = neighbor.build_lists(s)
    q_start = at.q.copy()
    charge_electrodes(at)
    pairs = neighbor.build_lists(dataclasses.replace(s, eletypes=None))[1]
    nall, n = at.nall, at.nlocal
    prd = tuple(float(p) for p in s.prd)
    lz = prd[2]
    rng = np.random.default_rng(24)
    image = rng.integers(-2, 3, (n, 3)).astype(np.int32)
    mass = np.resize(MASS, s.ntypes)
    m_atom = mass[at.type[:n] - 1]
    v0 = rng.normal(size=(n, 3)) * np.sqrt(BOLTZ * 298.0 / (m_atom * MVV2E))[:, None]
    fx = FixConp(s)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.pair_set_params(s.cutsq_table(), s.cutoff, lj_tables(s.ntypes, s.cutoff))
    fx.pair_set_list(pairs, nall)
    fx.integrate_set_params(at.type[:n], np.zeros(n, dtype=np.int32), mass, [0], [3.0 * n - 3.0], [100.0], 1.0, FTM2V, MVV2E, BOLTZ)
    fx.efield_set_params(np.ones(n, dtype=np.int32), QE2F, prd)
    d_x = torch.from_numpy(np.ascontiguousarray(at.x)).cuda()
    d_q = torch.from_numpy(at.q.copy()).cuda()
    d_im = torch.from_numpy(image).cuda()
    d_v = torch.from_numpy(v0).cuda()
    d_f = torch.zeros((nall, 3), dtype=torch.float64, device="cuda")
    d_out = torch.zeros(11, dtype=torch.float64, device="cuda")
    d_va = torch.zeros((n, 6), dtype=torch.float64, device="cuda")
    X, Q, IM, V, F, O, VA = (t.data_ptr() for t in (d_x, d_q, d_im, d_v, d_f, d_out, d_va))
    sync = torch.cuda.synchronize
    sync()
    fx.integrate_setup_device(V, np.array([298.0]))
    e = (0.0, 0.0, -1.0 / lz)
    rec = dict(box="headline", n_owned=int(n), n_selected=int(n), reps=args.reps, warmup=args.warmup)
    calls = {
        "forces": lambda: fx.efield_post_force_device(X, Q, F, e, d_image=IM),
        "forces_no_image": lambda: fx.efield_post_force_device(X, Q, F, e),
        "with_d_out": lambda: fx.efield_post_force_device(X, Q, F, e, d_image=IM, d_out=O),
        "with_vatom": lambda: fx.efield_post_force_device(X, Q, F, e, d_image=IM, d_vatom=VA),
        "with_d_out_and_vatom": lambda: fx.efield_post_force_device(X, Q, F, e, d_image=IM, d_out=O, d_vatom=VA),
    }
    for name, call in calls.items():
        rec[f"ms_{name}_wall"], rec[f"ms_{name}_host_thread"] = timed(call, args.reps, args.warmup, sync)
        rec[f"ms_{name}_device"] = device_ms(fx, "efield", call, sync)
    rec["d_out"] = [float(t) for t in d_out.cpu().numpy()]
    rec["ms_pair_device_forces_wall"], _ = timed(lambda: fx.pair_compute_device(X, Q, F, 0, 0, 0), max(args.reps // 10, 5), 3, sync)
    rec["ms_integrate_final_wall"], rec["ms_integrate_final_host_thread"] = timed(
        lambda: fx.integrate_final_device(V, F, 0), args.reps, args.warmup, sync)

    # the route without the entry: x, q and f down, q E in numpy, f up
    ez = QE2F * e[2]

    def host_route():
        hx, hq, hf = d_x.cpu().numpy(), d_q.cpu().numpy(), d_f.cpu().numpy()
        u = hx[:n, 2] + image[:, 2] * lz
        hf[:n, 2] += hq[:n] * ez
        energy = -float((hq[:n] * ez * u).sum())
        d_f.copy_(torch.from_numpy(hf))
        return energy
    rec["ms_host_route"], _ = timed(host_route, max(args.reps // 10, 5), 3, sync)
    fx.close()

    if not args.no_coupled:
        # a conq handle on the same box: the update, then the field that follows its scalar
        at.q[:] = q_start
        fq = FixConp(s, style="conq")
        fq.init_lists(alist, blist)
        fq.setup_post_neighbor(at)
        fq.setup_pre_force(at, 0, 0.35)
        fq.efield_set_params((at.echeck[:n] == 0).astype(np.int32), QE2F, prd)
        d_q.copy_(torch.from_numpy(at.q))
        d_f.zero_()
        reps = max(args.reps // 4, 10)

        def coupled():
            fq.pre_force_device(X, Q, 0.35)
            fq.efield_post_force_device(X, Q, F, (0.0, 0.0, 0.0), d_image=IM, couple=1, couple_scale=-1.0 / lz)

        def scalar_on_the_host():
            fq.pre_force_device(X, Q, 0.35)
            sc = fq.compute_scalar()
            fq.efield_post_force_device(X, Q, F, (0.0, 0.0, -sc / lz), d_image=IM)
        rec["ms_update_alone_wall"], rec["ms_update_alone_host_thread"] = timed(lambda: fq.pre_force_device(X, Q, 0.35), reps, 5, sync)
        rec["ms_update_then_coupled_wall"], rec["ms_update_then_coupled_host_thread"] = timed(coupled, reps, 5, sync)
        rec["ms_update_then_scalar_then_field_wall"], rec["ms_update_then_scalar_then_field_host_thread"] = timed(
            scalar_on_the_host, reps, 5, sync)
        rec["fix_scalar"] = fq.compute_scalar()
        fq.close()
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()
