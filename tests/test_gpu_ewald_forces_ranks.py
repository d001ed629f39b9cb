"""-m gpu: conp_ewald_compute_forces on spatially decomposed ranks (two / three processes share cuda:0, the conp_comm callbacks run
on torch.distributed gloo, as in tests/test_gpu_ewald_ranks.py): the structure factor and the sums of q, q^2, q z, q z^2 are
all-reduced, every rank returns the global energy and virial and the forces and per-atom energies of its own atoms.  Per tag they
equal the one-rank run to 1e-11 max|f| (1e-11 of the unsubtracted scale for the per-atom energies); E and W to 1e-12 of that scale."""
import os
import sys

import numpy as np
import pytest

import ewald_force_ref as ref
from conp_amd import FixConp, neighbor, systems

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
    f, E, W, e = fx.ewald_forces(at, eatom=True)                 # collective: forms S
    f2, E2, W2, e2 = fx.ewald_forces(at, eatom=True)             # collective: the cached S, the four sums again
    same = np.array_equal(f, f2) and E == E2 and np.array_equal(W, W2) and np.array_equal(e, e2)
    out[rank] = dict(f={int(t): [float(c) for c in v] for t, v in zip(at.tag[:n], f)}, e={int(t): float(v) for t, v in zip(at.tag[:n], e)},
                     q={int(t): float(v) for t, v in zip(at.tag[:n], at.q[:n])}, E=float(E), W=[float(v) for v in W], same=bool(same))
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
    f, E, W, e = fx.ewald_forces(at, eatom=True)
    T = ref.handle_tables(fx, s)
    scale = T["qs"] * ref.ksum(ref.structure_factor(np.ascontiguousarray(at.x[:n]), np.ascontiguousarray(at.q[:n]), T["kv"]), T["ug"])
    ref_f = {int(t): v for t, v in zip(at.tag[:n], f)}
    ref_e = {int(t): float(v) for t, v in zip(at.tag[:n], e)}
    fx.close()
    mgr = mp.Manager(); out = mgr.dict()
    port = 29600 + (os.getpid() + 11 * axis + world + 37) % 300
    mp.spawn(_worker, args=(world, port, name, axis, out), nprocs=world, join=True)
    got_f, got_e = {}, {}
    for r in range(world):
        assert out[r]["same"], r
        got_f.update(out[r]["f"]); got_e.update(out[r]["e"])
        dE, dW = abs(out[r]["E"] - E), np.abs(np.array(out[r]["W"]) - W).max()
        print(f"{name} rank {r}: |dE| {dE:.3e}, max |dW| {dW:.3e}, bound {1e-12 * scale:.3e}")
        assert dE <= 1e-12 * scale and dW <= 1e-12 * scale, (r, dE, dW, scale)
    assert sorted(got_f) == sorted(ref_f)
    fmax = np.abs(f).max()
    df = max(np.abs(np.array(got_f[t]) - ref_f[t]).max() for t in ref_f)
    de = max(abs(got_e[t] - ref_e[t]) for t in ref_e)
    print(f"{name}: max |df| {df:.3e} (bound {1e-11 * fmax:.3e}), max |de| {de:.3e} (bound {1e-11 * scale:.3e})")
    assert df <= 1e-11 * fmax and de <= 1e-11 * scale
