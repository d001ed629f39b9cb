"""-m gpu: the Ewald per-atom potential on spatially decomposed ranks (two / three processes share cuda:0, the conp_comm callbacks
run on torch.distributed gloo, as in tests/test_gpu_ranks.py): each rank contracts its own charged atoms, the structure factor is
all-reduced (km_ewald.cpp:784-785), each rank projects onto its own atoms.  The group potential per tag equals the one-rank run;
the per-atom entry is rank-local after a collective call and refuses after an update."""
import os
import sys

import numpy as np
import pytest

from conp_amd import ConpError, FixConp, neighbor, systems

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _make(name):
    return {"small_slab": lambda: systems.small_random(ne_side=4, n_elyte=96, lz=60.0, mode="slab"),
            "dilute_slab_generic": lambda: systems.deck("dilute", "slab", etypes=False)}[name]()


def _worker(rank, world, port, name, axis, out):
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(ROOT, "lammps-user-conp2_amd"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    s = _make(name)
    at, alist, blist = neighbor.build_lists_decomposed(s, world, axis=axis)[rank]
    fx = FixConp(s, device=0, rank=rank, nranks=world)
    fx.set_comm_torch()
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)
    n = at.nlocal
    pot = fx.ewald_group_potential(at, np.ones(n, np.int32))            # collective
    # rank r asks the per-atom entry r + 1 times after the collective compute: no collective inside, nothing hangs
    fx.ewald_compute(at)
    ok = [abs(fx.ewald_particle_potential(at, i) - (pot[i] + 2 * s.g_ewald * at.q[i] / np.sqrt(np.pi))) <= 1e-12 * max(1.0, abs(pot[i]))
          for i in range(min(rank + 1, n))]
    # an update drops the cache: the per-atom entry then refuses under ranks instead of starting a hidden collective
    fx.b_cal(at)
    refused = False
    try:
        fx.ewald_particle_potential(at, 0)
    except ConpError as e:
        refused = "collective" in str(e)
    out[rank] = dict(pot={int(t): float(v) for t, v in zip(at.tag[:n], pot)}, ok=all(ok) and len(ok) == min(rank + 1, n),
                     refused=refused)
    fx.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("name,axis,world", [("small_slab", 0, 2), ("dilute_slab_generic", 1, 3)])
def test_decomposed_ranks_match_one_rank(name, axis, world):
    import torch.multiprocessing as mp
    s = _make(name)
    at, alist, blist = neighbor.build_lists(s)
    fx = FixConp(s)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)
    n = at.nlocal
    ref = fx.ewald_group_potential(at, np.ones(n, np.int32))
    ref_t = {int(t): float(v) for t, v in zip(at.tag[:n], ref)}
    fx.close()
    mgr = mp.Manager(); out = mgr.dict()
    port = 29600 + (os.getpid() + 11 * axis + world + 150) % 300
    mp.spawn(_worker, args=(world, port, name, axis, out), nprocs=world, join=True)
    got = {}
    for r in range(world):
        assert out[r]["ok"] and out[r]["refused"], r
        got.update(out[r]["pot"])
    assert sorted(got) == sorted(ref_t)
    scale = max(abs(v) for v in ref_t.values())
    assert max(abs(got[t] - ref_t[t]) for t in ref_t) <= 1e-10 * scale
