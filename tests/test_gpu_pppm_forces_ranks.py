"""-m gpu: conp_pppm_compute_forces on spatially decomposed ranks (two / three processes share cuda:0, the conp_comm callbacks run on
torch.distributed gloo, as in tests/test_gpu_ewald_forces_ranks.py): one tagged gather of all ranks' charged atoms onto a replicated
mesh, the sums of q, q^2, q z, q z^2 all-reduced, every rank returns the global energy and virial -- bitwise equal across the ranks --
and the forces and per-atom energies of its own atoms.  Per tag they equal the one-rank run to 1e-10 max|f| (1e-11 of the
unsubtracted scale for the energies and the virial): the bounds of tests/test_gpu_pppm_forces.py."""
import os
import sys

import numpy as np
import pytest

from conp_amd import FixConp, neighbor, systems

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KW = dict(extra_args=["pppm"], pppm_mesh=(27, 24, 432), pppm_order=5)


def _make():
    return systems.deck("dilute", "slab", etypes=False)


def _worker(rank, world, port, axis, out):
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(ROOT, "lammps-user-conp2_amd"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    s = _make()
    at, alist, blist = neighbor.build_lists_decomposed(s, world, axis=axis)[rank]
    fx = FixConp(s, device=0, rank=rank, nranks=world, **KW)
    fx.set_comm_torch()
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)
    n = at.nlocal
    f, E, W, e = fx.pppm_compute_forces(at, eatom=True)
    out[rank] = dict(f={int(t): [float(c) for c in v] for t, v in zip(at.tag[:n], f)}, e={int(t): float(v) for t, v in zip(at.tag[:n], e)},
                     q={int(t): float(v) for t, v in zip(at.tag[:n], at.q[:n])}, E=float(E).hex(), W=[float(v).hex() for v in W])
    fx.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("axis,world", [(0, 2), (1, 3)])
def test_decomposed_ranks_match_one_rank(axis, world):
    import torch.multiprocessing as mp
    mgr = mp.Manager(); out = mgr.dict()
    port = 29600 + (os.getpid() + 11 * axis + world + 59) % 300
    mp.spawn(_worker, args=(world, port, axis, out), nprocs=world, join=True)
    got_f, got_e, got_q = {}, {}, {}
    for r in range(world):
        got_f.update(out[r]["f"]); got_e.update(out[r]["e"]); got_q.update(out[r]["q"])
        assert out[r]["E"] == out[0]["E"] and out[r]["W"] == out[0]["W"], r          # bit for bit
    # the one-rank run at the charges the ranks' update produced (the updates agree to the tolerance of tests/test_gpu_ranks.py only)
    s = _make()
    at, alist, blist = neighbor.build_lists(s)
    fx = FixConp(s, **KW)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)
    n = at.nlocal
    assert sorted(got_q) == sorted(int(t) for t in at.tag[:n])
    q1 = at.q[:n].copy()
    at.q[:n] = [got_q[int(t)] for t in at.tag[:n]]
    assert np.abs(at.q[:n] - q1).max() <= 1e-8 * np.abs(q1).max()
    f, E, W, e = fx.pppm_compute_forces(at, eatom=True)
    fx.close()
    # the unsubtracted scale qs (V / 2) sum G |rho^|^2 / N^2 = E + qs [g Q2 / sqrt(pi) + (pi / 2) Q^2 / (g^2 V)] - the slab energy
    x, q, g = at.x[:n], at.q[:n], s.g_ewald
    L = float(s.prd[2] * s.slab_volfactor)
    V = float(s.prd[0] * s.prd[1]) * L
    Q, Q2, M, M2 = q.sum(), (q * q).sum(), (q * x[:, 2]).sum(), (q * x[:, 2] ** 2).sum()
    assert s.slabflag
    scale = E + systems.QQRD2E * (g * Q2 / np.sqrt(np.pi) + 0.5 * np.pi * Q * Q / (g * g * V)
                                  - 2 * np.pi * (M * M - Q * M2 - Q * Q * L * L / 12.0) / V)
    assert scale > 0
    E_r, W_r = float.fromhex(out[0]["E"]), np.array([float.fromhex(v) for v in out[0]["W"]])
    fmax = np.abs(f).max()
    df = max(np.abs(np.array(got_f[int(t)]) - f[i]).max() for i, t in enumerate(at.tag[:n]))
    de = max(abs(got_e[int(t)] - e[i]) for i, t in enumerate(at.tag[:n]))
    print(f"world {world}: max |df| {df:.3e} (bound {1e-10 * fmax:.3e}), max |de| {de:.3e}, |dE| {abs(E_r - E):.3e}, "
          f"max |dW| {np.abs(W_r - W).max():.3e} (bound {1e-11 * scale:.3e})")
    assert df <= 1e-10 * fmax and de <= 1e-11 * scale
    assert abs(E_r - E) <= 1e-11 * scale and np.abs(W_r - W).max() <= 1e-11 * scale
