"""The per-group thermo sums from device arrays, beside the route an engine has without the entry.

    python tools/observe_time.py [--reps N] [--warmup W]

The headline box of bench.py (4096 electrode + 32768 electrolyte atoms, 36864 owned), image counters in -2 .. 2, thermal velocities.
Three sets of overlapping groups: 16 (all, electrolyte, electrode, left, right, the four electrolyte types, seven slabs of the
electrolyte along z), the 5 of the IL decks (sol, eleleft, eleright, ele, all) and 1 (all).  After W warm-up calls each, N calls
enqueued back to back with ONE synchronisation behind the last (wall = (enqueue + the final wait) / N, host = the enqueue loop
alone / N); then 50 calls with an event pair around each (conp_fix_profile: device = the time between the events, both launches):
  - conp_observe_device with d_v and d_image, without d_v, without d_image, without both;
  - for scale conp_integrate_temperature_device (one group of all atoms) and conp_pair_compute_device (forces only);
  - the host route the entry replaces: x, q and v down, the sums in numpy.
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

FTM2V = 1.0 / 48.88821291 / 48.88821291
MVV2E = 48.88821291 * 48.88821291
BOLTZ = 0.0019872067
MASS = np.array([67.07, 15.04, 57.12, 144.96, 12.001])


def group_sets(at, s, n):
    """-> {name: (ngroups, mask [n])}"""
    ech, typ, z = at.echeck[:n], at.type[:n], at.x[:n, 2]
    elyte = ech == 0
    five = [elyte, ech == 1, ech == -1, ech != 0, np.ones(n, dtype=bool)]
    etypes = np.unique(typ[elyte])
    by_type = [elyte & (typ == t) for t in np.resize(etypes, 4)]
    edges = np.linspace(z[elyte].min(), z[elyte].max() + 1e-9, 8)
    slabs = [elyte & (z >= edges[k]) & (z < edges[k + 1]) for k in range(7)]
    sixteen = [five[4], five[0], five[3], five[1], five[2]] + by_type + slabs

    def mask(members):
        m = np.zeros(n, dtype=np.int32)
        for g, mem in enumerate(members):
            m |= mem.astype(np.int32) << g
        return len(members), m
    return {"16_groups": mask(sixteen), "5_groups": mask(five), "1_group": mask([five[4]])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("observe_time.py: no GPU")
    torch.cuda.init()
    from conp_amd import FixConp, neighbor
    from bonded_time import timed
    from efield_time import device_ms
    from pair_time import lj_tables
    from pppm_force_time import box, charge_electrodes
    s, _mesh, _order = box("headline")
    at, alist, blist = neighbor.build_lists(s)
    charge_electrodes(at)
    pairs = neighbor.build_lists(dataclasses.replace(s, eletypes=None))[1]
    nall, n = at.nall, at.nlocal
    prd = tuple(float(p) for p in s.prd)
    rng = np.random.default_rng(25)
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
    d_x = torch.from_numpy(np.ascontiguousarray(at.x)).cuda()
    d_q = torch.from_numpy(at.q.copy()).cuda()
    d_im = torch.from_numpy(image).cuda()
    d_v = torch.from_numpy(v0).cuda()
    d_f = torch.zeros((nall, 3), dtype=torch.float64, device="cuda")
    d_out = torch.zeros((16, 10), dtype=torch.float64, device="cuda")
    d_t = torch.zeros((1, 4), dtype=torch.float64, device="cuda")
    X, Q, IM, V, F, O, T = (t.data_ptr() for t in (d_x, d_q, d_im, d_v, d_f, d_out, d_t))
    sync = torch.cuda.synchronize
    sync()
    rec = dict(box="headline", n_owned=int(n), reps=args.reps, warmup=args.warmup, library=os.environ.get("CONP_LIB", "product"))
    sets = group_sets(at, s, n)
    for name, (G, mask) in sets.items():
        fx.observe_set_params(at.type[:n], mask, mass, G, prd)
        calls = {"v_image": lambda: fx.observe_device(X, Q, O, d_v=V, d_image=IM)}
        if name == "16_groups":
            calls.update({"no_v": lambda: fx.observe_device(X, Q, O, d_image=IM), "no_image": lambda: fx.observe_device(X, Q, O, d_v=V),
                          "no_v_no_image": lambda: fx.observe_device(X, Q, O)})
        for cname, call in calls.items():
            key = f"ms_{name}_{cname}"
            rec[f"{key}_wall"], rec[f"{key}_host_thread"] = timed(call, args.reps, args.warmup, sync)
            rec[f"{key}_device"] = device_ms(fx, "observe", call, sync)
        fx.observe_device(X, Q, O, d_v=V, d_image=IM)
        rec[f"members_{name}"] = [int(t) for t in d_out.cpu().numpy()[:G, 0]]
    rec["ms_integrate_temperature_wall"], rec["ms_integrate_temperature_host_thread"] = timed(
        lambda: fx.integrate_temperature_device(V, T), args.reps, args.warmup, sync)
    rec["ms_integrate_temperature_device"] = device_ms(fx, "integrate", lambda: fx.integrate_temperature_device(V, T), sync)
    rec["ms_pair_device_forces_wall"], _ = timed(lambda: fx.pair_compute_device(X, Q, F, 0, 0, 0), max(args.reps // 10, 5), 3, sync)

    # the route without the entry: x, q and v down, the sums of the 16 groups in numpy
    G, mask = sets["16_groups"]
    lz = np.asarray(prd)

    def host_route():
        hx, hq, hv = d_x.cpu().numpy()[:n], d_q.cpu().numpy()[:n], d_v.cpu().numpy()
        u = hx + image * lz
        cols = np.column_stack([np.ones(n), hq, hq[:, None] * u, m_atom * (hv * hv).sum(axis=1), m_atom[:, None] * hv, m_atom])
        member = ((mask[:, None] >> np.arange(G)[None, :]) & 1).astype(np.float64)
        return member.T @ cols
    rec["ms_host_route"], _ = timed(host_route, max(args.reps // 10, 5), 3, sync)
    fx.observe_set_params(at.type[:n], mask, mass, G, prd)
    fx.observe_device(X, Q, O, d_v=V, d_image=IM)
    got, want = d_out.cpu().numpy(), host_route()
    rec["largest_difference_to_the_host_route"] = float(np.abs(got - want).max() / np.abs(want).max())
    print(json.dumps(rec), flush=True)
    fx.close()


if __name__ == "__main__":
    main()
