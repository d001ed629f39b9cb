"""The dihedral and improper forces of a step from device arrays, beside the bonded entry's time in the same process (DESIGN.md
section 28).

    python tools/dihedral_time.py [--reps N] [--warmup W]

The headline box of bench.py (4096 electrode + 32768 electrolyte atoms, ffield).  The 32768 electrolyte atoms are grouped eight at a
time into chains (4096 chains: 7 bonds, 6 angles, 5 dihedrals and 1 improper each; owned indices and the box lengths, the
closest-image form); the atoms of a chain are placed 1.5 A apart at 110 degrees with random torsions from its first atom on, so that
the terms are of an all-atom deck's size.  The handle runs on a stream of its own; after W warm-up calls each, N calls are enqueued
back to back between two events on that stream (ms = the events' elapsed time / N), split by outputs: forces only; forces and d_ev;
forces, d_ev, eatom and vatom -- for conp_dihedral_compute_device, for conp_bonded_compute_device over the same chains, and for the
host entry conp_dihedral_compute (the route the device entry removes: coordinates up, forces down).  Prints one JSON line.
Needs a GPU: there is no fall-back."""
import argparse
import dataclasses
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "lammps-user-conp2_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

CHAIN = 8


def chains(s, seed=3):
    """-> (x with the atoms of every chain placed behind its first atom and wrapped, bonds, angles, dihedrals, impropers)"""
    el = np.nonzero(s.echeck == 0)[0]
    mol = el[:len(el) // CHAIN * CHAIN].reshape(-1, CHAIN)
    n = len(mol)
    rng = np.random.default_rng(seed)
    unit = lambda v: v / np.linalg.norm(v, axis=1)[:, None]
    r, th = 1.5, np.deg2rad(110.0)
    pos = np.zeros((n, CHAIN, 3))
    pos[:, 0] = s.x[mol[:, 0]]
    u = unit(rng.normal(size=(n, 3)))
    pos[:, 1] = pos[:, 0] + r * u
    e1 = unit(np.cross(u, rng.normal(size=(n, 3))))
    for k in range(2, CHAIN):                            # atom k from the two before it: bond angle th, torsion random
        e2 = np.cross(u, e1)
        ph = rng.uniform(-np.pi, np.pi, (n, 1))
        w = -np.cos(th) * u + np.sin(th) * (np.cos(ph) * e1 + np.sin(ph) * e2)
        pos[:, k] = pos[:, k - 1] + r * w
        e1 = unit(np.cross(np.cross(u, w), w))
        u = w
    x = s.x.copy()
    x[mol.reshape(-1)] = pos.reshape(-1, 3)
    for c in range(3):
        if s.periodic[c]:
            x[:, c] = s.boxlo[c] + np.mod(x[:, c] - s.boxlo[c], s.prd[c])
    one = np.ones(n, dtype=np.int32)
    bonds = np.concatenate([np.stack([mol[:, k], mol[:, k + 1], one], 1) for k in range(CHAIN - 1)])
    angles = np.concatenate([np.stack([mol[:, k], mol[:, k + 1], mol[:, k + 2], one], 1) for k in range(CHAIN - 2)])
    dihedrals = np.concatenate([np.stack([mol[:, k], mol[:, k + 1], mol[:, k + 2], mol[:, k + 3], one], 1) for k in range(CHAIN - 3)])
    impropers = np.stack([mol[:, 1], mol[:, 0], mol[:, 2], mol[:, 3], one], 1)
    return np.ascontiguousarray(x), bonds, angles, dihedrals, impropers


def timed(call, reps, warmup, stream):
    import torch
    for _ in range(warmup):
        call()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream.synchronize()
    a.record(stream)
    for _ in range(reps):
        call()
    b.record(stream)
    b.synchronize()
    return round(a.elapsed_time(b) / reps, 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("dihedral_time.py: no GPU")
    torch.cuda.init()
    from conp_amd import FixConp, neighbor
    from pppm_force_time import box
    s, _mesh, _order = box("headline")
    at = neighbor.make_ghosts(s)
    nall, n = at.nlocal + at.nghost, at.nlocal
    fx = FixConp(s)
    stream = torch.cuda.Stream()
    fx.set_stream(stream.cuda_stream)
    xm, bonds, angles, dihedrals, impropers = chains(s)
    xb = at.x.copy(); xb[:n] = xm                                                # (ghost rows are not read: owned indices)
    prd = np.where(s.periodic, s.prd, 0.0)
    fx.bonded_set_params([310.0], [1.5], [58.0], [np.deg2rad(110.0)], newton_bond=True)
    fx.bonded_set_lists(n, nall, bonds, angles, prd)
    fx.dihedral_set_params("opls", [[1.3, -0.05, 0.2, 0.0]], "harmonic", [[2.1, 0.0]], newton_bond=True)
    fx.dihedral_set_lists(n, nall, dihedrals, impropers, prd)
    atb = dataclasses.replace(at, x=np.ascontiguousarray(xb))
    f = np.zeros((nall, 3))
    d_xb = torch.from_numpy(atb.x).cuda()
    d_f = torch.zeros((nall, 3), dtype=torch.float64, device="cuda")
    d_ev = torch.zeros(8, dtype=torch.float64, device="cuda")
    d_e = torch.zeros(nall, dtype=torch.float64, device="cuda")
    d_v = torch.zeros((nall, 6), dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    outputs = {"forces": (False, False), "forces_ev": (True, False), "forces_ev_atom": (True, True)}
    rec = dict(box="headline", n_owned=int(n), n_all=int(nall), chains=len(impropers), bonds=len(bonds), angles=len(angles),
               dihedrals=len(dihedrals), impropers=len(impropers), reps=args.reps, warmup=args.warmup)
    for name, (ev, atom) in outputs.items():
        outs = (d_f.data_ptr(), d_ev.data_ptr() if ev else 0, d_e.data_ptr() if atom else 0, d_v.data_ptr() if atom else 0)

        def dihedral():
            fx.dihedral_compute_device(d_xb.data_ptr(), *outs)

        def bonded():
            fx.bonded_compute_device(d_xb.data_ptr(), *outs)

        def host():
            fx.dihedral_compute(atb, f=f, eng=ev, virial=ev, eatom=atom, vatom=atom)
        rec[f"ms_dihedral_device_{name}"] = timed(dihedral, args.reps, args.warmup, stream)
        rec[f"ms_bonded_device_{name}"] = timed(bonded, args.reps, args.warmup, stream)
        rec[f"ms_dihedral_host_{name}"] = timed(host, args.reps, args.warmup, stream)
    print(json.dumps(rec), flush=True)
    fx.close()


if __name__ == "__main__":
    main()
