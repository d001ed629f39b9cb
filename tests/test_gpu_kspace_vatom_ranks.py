"""-m gpu: the per-atom virial of the host entries on spatially decomposed ranks (two processes share cuda:0, the conp_comm
callbacks run on torch.distributed gloo, as in tests/test_gpu_ewald_forces_ranks.py / tests/test_gpu_pppm_forces_ranks.py), one deck
per provider.  S / the mesh is global already, so the per-atom virial needs no collective of its own: per tag every rank's vatom rows
equal the one-rank run at the same charges within 1e-11 of the unsubtracted scale."""
import os
import sys

import numpy as np
import pytest

import ewald_force_ref as ref
from conp_amd import FixConp, neighbor, systems

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = {"ewald": {}, "pppm": dict(extra_args=["pppm"], pppm_mesh=(27, 24, 432), pppm_order=5)}


def _make(provider):
    if provider == "ewald":
        return systems.small_random(ne_side=4, n_elyte=96, lz=60.0, mode="slab")
    return systems.deck("dilute", "slab", etypes=False)


def _entry(fx, provider):
    return fx.ewald_forces_vatom if provider == "ewald" else fx.pppm_forces_vatom


def _worker(rank, world, port, provider, out):
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(ROOT, "lammps-user-conp2_amd"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    s = _make(provider)
    at, alist, blist = neighbor.build_lists_decomposed(s, world, axis=0)[rank]
    fx = FixConp(s, device=0, rank=rank, nranks=world, **KW[provider])
    fx.set_comm_torch()
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)
    n = at.nlocal
    f, E, W, e, v = _entry(fx, provider)(at, eatom=True)            # collective, as the sibling is
    out[rank] = dict(v={int(t): [float(c) for c in r] for t, r in zip(at.tag[:n], v)},
                     q={int(t): float(c) for t, c in zip(at.tag[:n], at.q[:n])}, W=[float(c) for c in W])
    fx.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("provider", ["ewald", "pppm"])
def test_decomposed_ranks_return_the_one_rank_vatom(provider):
    import torch.multiprocessing as mp
    world = 2
    mgr = mp.Manager(); out = mgr.dict()
    port = 29600 + (os.getpid() + world + (71 if provider == "ewald" else 83)) % 300
    mp.spawn(_worker, args=(world, port, provider, out), nprocs=world, join=True)
    got_v, got_q = {}, {}
    for r in range(world):
        got_v.update(out[r]["v"]); got_q.update(out[r]["q"])
    # the one-rank run at the charges the ranks' update produced
    s = _make(provider)
    at, alist, blist = neighbor.build_lists(s)
    fx = FixConp(s, **KW[provider])
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)
    n = at.nlocal
    assert sorted(got_q) == sorted(int(t) for t in at.tag[:n])
    q1 = at.q[:n].copy()
    at.q[:n] = [got_q[int(t)] for t in at.tag[:n]]
    assert np.abs(at.q[:n] - q1).max() <= 1e-8 * np.abs(q1).max()
    x, q, g = np.ascontiguousarray(at.x[:n]), np.ascontiguousarray(at.q[:n]), s.g_ewald
    if provider == "ewald":
        fx.ewald_compute(at)
        T = ref.handle_tables(fx, s)
        scale = T["qs"] * ref.ksum(ref.structure_factor(x, q, T["kv"]), T["ug"])
    f, E, W, e, v = _entry(fx, provider)(at, eatom=True)
    fx.close()
    if provider == "pppm":      # qs (V / 2) sum G |rho^|^2 / N^2 from the energy (tests/test_gpu_pppm_forces_ranks.py)
        L = float(s.prd[2] * s.slab_volfactor)
        V = float(s.prd[0] * s.prd[1]) * L
        Q, Q2, M, M2 = q.sum(), (q * q).sum(), (q * x[:, 2]).sum(), (q * x[:, 2] ** 2).sum()
        assert s.slabflag
        scale = E + systems.QQRD2E * (g * Q2 / np.sqrt(np.pi) + 0.5 * np.pi * Q * Q / (g * g * V)
                                      - 2 * np.pi * (M * M - Q * M2 - Q * Q * L * L / 12.0) / V)
    assert scale > 0 and np.abs(v).max() > 0
    dv = max(np.abs(np.array(got_v[int(t)]) - v[i]).max() for i, t in enumerate(at.tag[:n]))
    print(f"{provider}, {world} ranks: max |dvatom| {dv:.3e}, bound {1e-11 * scale:.3e} ({dv / (1e-11 * scale):.3g} of it)")
    assert dv <= 1e-11 * scale
    part = np.sum([out[rr]["v"][t] for rr in range(world) for t in out[rr]["v"]], axis=0)        # all ranks' rows add up to the
    for r in range(world):                                         # global virial every rank returned
        assert np.abs(part - np.array(out[r]["W"])).max() <= 1e-11 * scale
