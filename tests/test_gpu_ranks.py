"""-m gpu: several ranks.  (1) spatially decomposed atoms with the conp_comm callbacks (the LAMMPS-MPI route; here two / three
processes share cuda:0 and the callbacks run on torch.distributed gloo) against the one-rank result; (2) the RCCL data plane
inside the library -- a one-rank communicator exercises every RCCL call site (all-reduce of b and of the sharded A build,
in-place all-gather of q, row-sharded S and its re-assembly) on the one GPU this box has; several GPUs are the driver's bench;
(3) the sharded A build on decks with 28 and 210 tiles, two and three ranks.  Out of scope: the by_range real-space split of a_cal
(can_exchange() && !decomposed) exists only under a multi-rank RCCL communicator, which one GPU cannot form."""
import os
import sys

import numpy as np
import pytest

from conp_amd import FixConp, neighbor, systems
from helpers import rel_err

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _make(name):
    import dataclasses
    newton = name.endswith("_newton")          # `newton on`: owned-ghost pairs are listed ONCE, by one of the two ranks
    s = {"small_slab": lambda: systems.small_random(ne_side=4, n_elyte=96, lz=60.0, mode="slab"),
         "dilute_ffield": lambda: systems.deck("dilute", "ffield", etypes=True),
         "dilute_slab_generic": lambda: systems.deck("dilute", "slab", etypes=False)}[name.replace("_newton", "")]()
    return dataclasses.replace(s, newton=True) if newton else s


def _extras(solver):
    # "pppm": the k-space b from the device mesh (rank 0 owns it; the ranks' charged electrolyte atoms are gathered like for Ewald)
    return {"inv": {}, "cg": dict(extra_args=["cg"]), "pppm": dict(extra_args=["pppm"], pppm_mesh=(27, 24, 144), pppm_order=5)}[solver]


def _decomposed_worker(rank, world, port, name, axis, solver, out):
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(ROOT, "lammps-user-conp2_amd"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    s = _make(name)
    at, alist, blist = neighbor.build_lists_decomposed(s, world, axis=axis)[rank]
    fx = FixConp(s, device=0, rank=rank, nranks=world, **_extras(solver))
    fx.set_comm_torch()
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)
    q0 = {int(t): float(q) for t, q, e in zip(at.tag[:at.nlocal], at.q[:at.nlocal], at.echeck[:at.nlocal]) if e}
    sc0 = fx.compute_scalar()
    # a second update with changed electrolyte charges (the per-step gather), and the post-force correction
    sol = at.echeck == 0
    at.q[sol] *= 1.25
    fx.pre_force(at, 1, 0.4)
    q1 = {int(t): float(q) for t, q, e in zip(at.tag[:at.nlocal], at.q[:at.nlocal], at.echeck[:at.nlocal]) if e}
    f, ek, ec, vir = fx.post_force(at)
    S = fx.matrix() if solver != "cg" else None             # collective: the row-sharded inverse is re-assembled
    m = fx.maps()
    mesh = None
    if solver == "pppm":
        # PPPMCONP's coupling beyond b under decomposition (pppm_conp.cpp:385-534): the density brick of ALL atoms and the mesh
        # potentials of this rank's electrode atoms -- collective calls, every rank gathers all charged atoms onto its mesh copy
        nfft = 27 * 24 * 144
        rho, rho_e, rho_l = fx.pppm_make_rho(at, nfft)
        sel = (at.echeck[:at.nlocal] != 0).astype(np.int32)
        pot = fx.pppm_group_potential(at, sel)
        # compute potential/atom's k-space part on the mesh handle: collective too (its own spread of all ranks' atoms, the slab
        # sums all-reduced), the values of this rank's electrode atoms
        patom = fx.compute_potential_atom(at, blist, np.ones(at.nlocal + at.nghost, np.int32), pair=False, kspace=True, qsum=True)
        # the per-atom entry is RANK-LOCAL (pppm_conp.cpp:452-485: compute potential/atom calls it once per owned group atom, a
        # different number of times on every rank): rank r asks r + 1 times after the collective entry above left the brick --
        # no collective inside, so nothing hangs --, and each value is the group entry's + 2 g q / sqrt(pi)
        idx = np.nonzero(sel)[0]
        n_before = fx.info().pppm_elyte_spreads
        per_atom = []
        for i in idx[:rank + 1]:
            u = fx.pppm_particle_potential(at, int(i))
            per_atom.append(abs(u - (pot[i] + 2.0 * s.g_ewald * at.q[i] / np.sqrt(np.pi))) <= 1e-12 * max(1.0, abs(u)))
        assert fx.info().pppm_elyte_spreads == n_before and all(per_atom) and len(per_atom) == min(rank + 1, len(idx))
        # an update invalidates the brick: the per-atom entry then REFUSES under ranks instead of starting a hidden collective
        refused = False
        fx.b_cal(at)
        try:
            if len(idx): fx.pppm_particle_potential(at, int(idx[0]))
        except Exception as e:
            refused = "collective" in str(e)
        assert refused or not len(idx)
        mesh = dict(rho=rho, rho_e=rho_e, pot={int(t): float(v) for t, v, e in zip(at.tag[:at.nlocal], pot, sel) if e},
                    patom={int(t): float(v) for t, v, e in zip(at.tag[:at.nlocal], patom, sel) if e})
    out[rank] = dict(q0=q0, q1=q1, sc0=sc0, sc1=fx.compute_scalar(), ek=ek, S=S, eleall2tag=m["eleall2tag"].copy(), mesh=mesh,
                     info=(fx.info().elenum, fx.info().elenum_all, fx.info().n_elyte_charged))
    fx.close()
    dist.destroy_process_group()


# the *_newton cases: contributions to an electrode atom that is a GHOST on the rank that lists the pair -- the reference's
# newtonbuf + MPI_Allreduce route (fix_conp.cpp:1311, 1345-1361); here they travel in the all-reduce of b / of the A build
@pytest.mark.parametrize("name,axis,world,solver", [("small_slab", 0, 2, "inv"), ("dilute_ffield", 2, 2, "inv"),
                                                    ("dilute_slab_generic", 1, 3, "inv"), ("small_slab", 1, 2, "cg"),
                                                    ("small_slab_newton", 0, 2, "inv"), ("dilute_ffield_newton", 2, 2, "inv"),
                                                    ("dilute_slab_generic_newton", 1, 3, "inv"),
                                                    ("dilute_ffield", 2, 2, "pppm"), ("dilute_slab_generic", 0, 3, "pppm")])
def test_decomposed_ranks_match_one_rank(name, axis, world, solver):
    import torch.multiprocessing as mp
    s = _make(name)
    at, alist, blist = neighbor.build_lists(s)
    fx = FixConp(s, **_extras(solver))
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)
    ele = at.echeck[:at.nlocal] != 0
    q0 = {int(t): float(q) for t, q in zip(at.tag[:at.nlocal][ele], at.q[:at.nlocal][ele])}
    sc0 = fx.compute_scalar()
    at.q[at.echeck == 0] *= 1.25
    fx.pre_force(at, 1, 0.4)
    q1 = {int(t): float(q) for t, q in zip(at.tag[:at.nlocal][ele], at.q[:at.nlocal][ele])}
    sc1 = fx.compute_scalar()
    _, ek, _, _ = fx.post_force(at)
    S1 = fx.matrix()
    tags1 = fx.maps()["eleall2tag"]
    n_charged = fx.info().n_elyte_charged
    mesh1 = None
    if solver == "pppm":
        rho, rho_e, _ = fx.pppm_make_rho(at, 27 * 24 * 144)
        sel = (at.echeck[:at.nlocal] != 0).astype(np.int32)
        pot = fx.pppm_group_potential(at, sel)
        patom = fx.compute_potential_atom(at, blist, np.ones(at.nlocal + at.nghost, np.int32), pair=False, kspace=True, qsum=True)
        mesh1 = dict(rho=rho, rho_e=rho_e, pot={int(t): float(v) for t, v, e in zip(at.tag[:at.nlocal], pot, sel) if e},
                     patom={int(t): float(v) for t, v, e in zip(at.tag[:at.nlocal], patom, sel) if e})
    fx.close()
    mgr = mp.Manager(); out = mgr.dict()
    port = 29600 + (os.getpid() + 7 * axis + world) % 300
    mp.spawn(_decomposed_worker, args=(world, port, name, axis, solver, out), nprocs=world, join=True)
    tol = 1e-6 if solver == "cg" else 1e-9
    allq0, allq1 = {}, {}
    for r in range(world):
        o = out[r]
        assert not (set(o["q0"]) & set(allq0))                      # every electrode atom has one owner
        allq0.update(o["q0"]); allq1.update(o["q1"])
        assert o["info"][1] == len(q0) and o["info"][2] == n_charged
        assert o["sc0"] == pytest.approx(sc0, rel=tol, abs=1e-12) and o["sc1"] == pytest.approx(sc1, rel=tol, abs=1e-12)
        assert o["ek"] == pytest.approx(ek, rel=1e-9)                # self energy: sum over the electrode atoms of ALL ranks
    assert sorted(allq0) == sorted(q0)
    scale = max(abs(v) for v in q0.values())
    assert max(abs(allq0[t] - q0[t]) for t in q0) < tol * scale
    assert max(abs(allq1[t] - q1[t]) for t in q1) < tol * scale
    if solver == "pppm":
        # every rank holds the whole mesh: the same bricks as one rank (the spread adds in another order: f64 atomics), and the
        # potentials of its own electrode atoms
        allpot, allpatom = {}, {}
        for r in range(world):
            mr = out[r]["mesh"]
            assert rel_err(mr["rho"], mesh1["rho"]) < 1e-12 and rel_err(mr["rho_e"], mesh1["rho_e"]) < 1e-12
            assert not (set(mr["pot"]) & set(allpot))
            allpot.update(mr["pot"]); allpatom.update(mr["patom"])
        assert sorted(allpot) == sorted(mesh1["pot"]) and sorted(allpatom) == sorted(mesh1["patom"])
        pscale = max(abs(v) for v in mesh1["pot"].values())
        assert max(abs(allpot[t] - mesh1["pot"][t]) for t in allpot) < 1e-10 * pscale
        # potential/atom on the mesh handle (with the slab sums of all ranks in the slab case): the one-rank values, by tag
        ascale = max(abs(v) for v in mesh1["patom"].values())
        assert ascale > 0
        assert max(abs(allpatom[t] - mesh1["patom"][t]) for t in allpatom) < 1e-10 * ascale
    if solver != "cg":
        # the projected inverse in the ranks' own (rank-major) numbering == the one-rank matrix permuted by tag
        pos1 = {int(t): i for i, t in enumerate(tags1)}
        perm = np.array([pos1[int(t)] for t in out[0]["eleall2tag"]])
        for r in range(world):
            assert np.array_equal(out[r]["eleall2tag"], out[0]["eleall2tag"])
            assert rel_err(out[r]["S"], S1[np.ix_(perm, perm)]) < 1e-8


def _make_tiled(name):
    """decks whose electrode spans many 128 x 128 tiles, so that the cyclic dealing gives every rank several"""
    import dataclasses
    from test_gpu_parity import rough
    base = name.replace("_newton", "")
    s = {"il_onelayer_ffield": lambda: systems.deck("il_onelayer", "ffield"),                       # 832 atoms: 28 tiles, z-class kernel
         "il_onelayer_rough": lambda: rough(systems.deck("il_onelayer", "ffield")),                 # general kernel + nsplit
         "cond2_ffield": lambda: systems.deck("cond2", "ffield")}[base]()          # 2496 atoms: 210 tiles, 52 z values -> general kernel
    return dataclasses.replace(s, newton=True) if name.endswith("_newton") else s


def _tiled_worker(rank, world, port, name, axis, out):
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(ROOT, "lammps-user-conp2_amd"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    s = _make_tiled(name)
    at, alist, blist = neighbor.build_lists_decomposed(s, world, axis=axis)[rank]
    fx = FixConp(s, device=0, rank=rank, nranks=world)
    fx.set_comm_torch()
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.a_cal(at)                                # tiles rank, rank + world, ...; diagonal and slab term on rank 0; all-reduce inside
    A = fx.matrix()
    nzc = fx.info().n_zclasses
    fx.close()
    # (a handle whose A was built by hand has left the setup stage: the hooks run on a fresh one, all ranks in step)
    fx = FixConp(s, device=0, rank=rank, nranks=world)
    fx.set_comm_torch()
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)
    at.q[at.echeck == 0] *= 1.25
    fx.pre_force(at, 1, 0.4)
    q = {int(t): float(v) for t, v, e in zip(at.tag[:at.nlocal], at.q[:at.nlocal], at.echeck[:at.nlocal]) if e}
    out[rank] = dict(A=A, q=q, sc=fx.compute_scalar(), eleall2tag=fx.maps()["eleall2tag"].copy(), elenum=fx.info().elenum, nzc=nzc)
    fx.close()
    dist.destroy_process_group()


# (the third case splits along z in three: the middle rank holds electrolyte only -- it owns no electrode atom and no real-space
# row, and still builds its share of the k-space tiles)
@pytest.mark.parametrize("name,axis,world,nzc,tiles,every_rank_owns_electrode", [
    ("il_onelayer_ffield", 0, 2, 2, 28, True), ("il_onelayer_ffield", 2, 3, 2, 28, False), ("il_onelayer_rough", 1, 3, 0, 28, True),
    ("cond2_ffield", 0, 2, 52, 210, True), ("il_onelayer_ffield_newton", 0, 2, 2, 28, True)],
    ids=["il_onelayer-x2", "il_onelayer-z3_middle_rank_without_electrode_atoms", "il_onelayer_rough-y3", "cond2-x2",
         "il_onelayer_newton-x2"])
def test_sharded_a_build_with_several_tiles_per_rank(name, axis, world, nzc, tiles, every_rank_owns_electrode):
    """RankExchange::can_exchange(): the lower-triangle tiles of A dealt cyclically to 2 / 3 ranks (tile_first = rank, tile_stride = nranks),
    diagonal and slab term on rank 0 only, real-space rows by owner, the partial matrices summed through conp_comm -- on decks with
    28 and 210 tiles, where every rank really gets several.  Every element is written by one rank's tile and at most one rank's
    real-space row, so each rank's A must be the one-rank A (permuted by tag) to rounding of the row sums: 1e-11 of the largest
    entry (TOL_A); then the setup is finished and one update made: charges and scalar to 1e-9 as in the test above.
    Not covered: the by_range real-space split (can_exchange() && !decomposed) only exists under a multi-rank RCCL communicator,
    which one GPU cannot form."""
    import torch.multiprocessing as mp
    s = _make_tiled(name)
    at, alist, blist = neighbor.build_lists(s)
    fx = FixConp(s)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.a_cal(at)
    A1 = fx.matrix()
    ne = A1.shape[0]
    nb = (ne + 127) // 128
    assert fx.info().n_zclasses == nzc and nb * (nb + 1) // 2 == tiles and tiles >= 4 * world
    fx.close()
    fx = FixConp(s)
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.setup_pre_force(at, 0, s.potdiff)
    at.q[at.echeck == 0] *= 1.25
    fx.pre_force(at, 1, 0.4)
    ele = at.echeck[:at.nlocal] != 0
    q1 = {int(t): float(q) for t, q in zip(at.tag[:at.nlocal][ele], at.q[:at.nlocal][ele])}
    sc1 = fx.compute_scalar()
    tags1 = fx.maps()["eleall2tag"]
    fx.close()
    mgr = mp.Manager(); out = mgr.dict()
    port = 29300 + (os.getpid() + 7 * axis + world) % 250
    mp.spawn(_tiled_worker, args=(world, port, name, axis, out), nprocs=world, join=True)
    res = [out[r] for r in range(world)]
    owns = [o["elenum"] for o in res]
    assert sum(owns) == ne
    if every_rank_owns_electrode:
        assert min(owns) > 0, owns
    else:
        assert owns[1] == 0 and owns[0] > 0 and owns[2] > 0, owns
    pos1 = {int(t): i for i, t in enumerate(tags1)}
    perm = np.array([pos1[int(t)] for t in res[0]["eleall2tag"]])
    A_ref = A1[np.ix_(perm, perm)]
    allq = {}
    for r, o in enumerate(res):
        assert np.array_equal(o["eleall2tag"], res[0]["eleall2tag"]) and o["nzc"] == nzc
        e_a = rel_err(o["A"], A_ref)
        print(f"{name} axis {axis} world {world} rank {r}: owns {o['elenum']} electrode atoms, A vs one rank {e_a:.2e} of max")
        assert e_a < 1e-11
        assert np.array_equal(o["A"], o["A"].T)
        assert o["sc"] == pytest.approx(sc1, rel=1e-9, abs=1e-12)
        assert not (set(o["q"]) & set(allq))
        allq.update(o["q"])
    assert sorted(allq) == sorted(q1)
    scale = max(abs(v) for v in q1.values())
    assert max(abs(allq[t] - q1[t]) for t in q1) < 1e-9 * scale


def _rccl_worker(rank, world, port, out):
    import torch
    import torch.distributed as dist
    sys.path.insert(0, os.path.join(ROOT, "lammps-user-conp2_amd"))
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    s = systems.deck("il_onelayer", "ffield")
    at, alist, blist = neighbor.build_lists(s)
    fx = FixConp(s, device=0, rank=rank, nranks=world)
    assert fx.comm_init_rccl()                                 # availability agreed, ncclGetUniqueId on rank 0, 128 bytes broadcast, ncclCommInitRank
    fx.init_lists(alist, blist)
    fx.setup_post_neighbor(at)
    fx.linalg_setup(at)                                        # tiles dealt to the ranks, all-reduce(A) on RCCL
    d_x = torch.from_numpy(np.ascontiguousarray(at.x)).cuda(); d_q = torch.from_numpy(at.q.copy()).cuda()
    for _ in range(3):
        fx.pre_force_device(d_x.data_ptr(), d_q.data_ptr(), s.potdiff)     # all-reduce(b), rows of S b, all-gather(q) inside
    torch.cuda.synchronize()
    b, q, _ = fx.vectors()
    out[rank] = (b, q, d_q.cpu().numpy(), fx.matrix())
    fx.close()
    dist.destroy_process_group()


def test_rccl_data_plane_one_rank_communicator():
    import torch.multiprocessing as mp
    s = systems.deck("il_onelayer", "ffield")
    at, alist, blist = neighbor.build_lists(s)
    fx = FixConp(s)
    fx.init_lists(alist, blist); fx.setup_post_neighbor(at); fx.setup_pre_force(at, 0, s.potdiff)
    b1, q1, _ = fx.vectors()
    S1 = fx.matrix()
    fx.close()
    mgr = mp.Manager(); out = mgr.dict()
    mp.spawn(_rccl_worker, args=(1, 29950 + os.getpid() % 40, out), nprocs=1, join=True)
    b, q, q_atoms, S = out[0]
    assert rel_err(b, b1) < 1e-12 and rel_err(q, q1) < 1e-11 and rel_err(S, S1) < 1e-12
    ele = at.echeck != 0
    assert rel_err(q_atoms[ele], at.q[ele]) < 1e-11
