// What the glue classes (FixConpHip, KSpaceModuleHip, PPPMConpHip, ComputePotentialAtomHip) share, each fact once: the error
// channel, the conp_env every handle starts from, the MPI-backed conp_comm, the conp_atoms view, and the handle of a k-space provider.
// Header-only; the callbacks themselves are in conp_mpi_comm.h.
#pragma once
#include <cstring>
#include <vector>

#include "conp_hip.h"
#include "conp_mpi_comm.h"
#ifdef CONP_GLUE_MOCK
#include "mock_lammps/lammps_mock.h"
#else
#include "atom.h"
#include "comm.h"
#include "domain.h"
#include "error.h"
#include "force.h"
#include "kspace.h"
#endif

namespace conp_glue {

inline void fail_if(LAMMPS_NS::Error *error, int status) {
  if (status != CONP_OK) error->all(FLERR, conp_last_error());   // the reference's only error channel (fix_conp.cpp:86,...)
}

// conp_env as far as every handle fills it the same way.  `ks`: where g_ewald & co. are read (km_ewald.cpp:66-69) -- force->kspace,
// or the pppm style itself.  cutsq, cut_coul, one_electrode, ghost_images and the pppm mesh are the caller's.
// Several MPI ranks (spatial decomposition): every rank drives its own handle on its own atoms and lists; device = -(2 + l) lets the
// library take GPU (l mod visible devices), so that the ranks of a NODE spread over its GPUs or share one.
inline conp_env base_env(LAMMPS_NS::Force *force, LAMMPS_NS::Domain *domain, LAMMPS_NS::Atom *atom, LAMMPS_NS::Comm *comm,
                         MPI_Comm world, LAMMPS_NS::KSpace *ks) {
  conp_env env;
  std::memset(&env, 0, sizeof(env));
  env.qqrd2e = force->qqrd2e; env.qqr2e = force->qqr2e; env.qe2f = force->qe2f; env.dielectric = force->dielectric;
  env.newton_pair = force->newton_pair;
  env.g_ewald = ks->g_ewald; env.accuracy = ks->accuracy; env.slab_volfactor = ks->slab_volfactor; env.slabflag = ks->slabflag;
  env.xprd = domain->xprd; env.yprd = domain->yprd; env.zprd = domain->zprd;
  env.boxlo_x = domain->boxlo[0]; env.boxlo_y = domain->boxlo[1]; env.boxlo_z = domain->boxlo[2];
  env.ntypes = atom->ntypes;
  env.device = comm->nprocs > 1 ? -(2 + node_local_rank(world)) : 0;
  env.rank = comm->me; env.nranks = comm->nprocs;
  return env;
}

// conp_comm on MPI: the collectives FixConp makes on `world` (fix_conp.cpp:415, 492, 523, 535, 643, 822, 1356; km_ewald.cpp:77,
// 784), handed to the library as callbacks right after conp_fix_create.  ctx = &world.  One rank: nothing to install.
inline int install_mpi_comm(conp_fix *h, MPI_Comm *world, int me, int nprocs) {
  if (nprocs == 1) return CONP_OK;
  conp_comm cc;
  cc.ctx = world; cc.rank = me; cc.nranks = nprocs;
  cc.allreduce_sum = cb_allreduce_sum; cc.allreduce_max_int = cb_allreduce_max_int;
  cc.allgather_int = cb_allgather_int; cc.allgatherv = cb_allgatherv;
  return conp_fix_set_comm(h, &cc);
}

// conp_atoms over LAMMPS' per-atom arrays.  `electrode`: electrode_check(i) of fix_conp.cpp:599-605, however the caller reaches it.
struct AtomView {
  std::vector<int> echeck;
  std::vector<double> xflat;
  // x in place: atom->x is a LAMMPS 2-d array (Memory::create), one contiguous [nmax][3] block behind the row pointers
  template <class F> conp_atoms in_place(LAMMPS_NS::Atom *atom, F electrode) {
    const int nall = atom->nlocal + atom->nghost;
    echeck.resize(nall);
    for (int i = 0; i < nall; ++i) echeck[i] = electrode(i);
    conp_atoms a;
    a.nlocal = atom->nlocal; a.nghost = atom->nghost; a.x = nall ? &atom->x[0][0] : nullptr; a.q = atom->q; a.type = atom->type;
    a.tag = atom->tag; a.echeck = echeck.data();
    return a;
  }
  // x as a flattened copy
  template <class F> conp_atoms flat(LAMMPS_NS::Atom *atom, F electrode) {
    conp_atoms a = in_place(atom, electrode);
    const int nall = a.nlocal + a.nghost;
    xflat.resize(3 * (size_t)nall);
    for (int i = 0; i < nall; ++i)
      for (int c = 0; c < 3; ++c) xflat[3 * (size_t)i + c] = atom->x[i][c];
    a.x = xflat.data();
    return a;
  }
};

// conp_fix_args of a provider's handle: the fix-side solver never runs on it; the caller adds eta and lowmem
inline conp_fix_args provider_args(int pppm) {
  conp_fix_args fa;
  std::memset(&fa, 0, sizeof(fa));
  fa.everynum = 1; fa.minimizer = CONP_SOLVER_INV; fa.maxiter = 100; fa.tolerance = 1e-6; fa.nullneutral = 1; fa.pppm = pppm;
  return fa;
}

// The conp_fix handle of a k-space provider (a member of KSpaceModuleHip and PPPMConpHip): created at conp_setup, it follows the
// fix's atoms through an empty neighbour list and serves a_cal / b_cal in the fix's own electrode numbering.  `Fix` is the
// reference's FixConp as far as a provider reads it (elenum, elenum_all, ele2tag, eleall2tag: fix_conp.h:58-89).
class ProviderHandle {
 public:
  conp_fix *h = nullptr;
  explicit ProviderHandle(LAMMPS_NS::Error *e) : error(e) {}
  ~ProviderHandle() { conp_fix_destroy(h); }

  void create(const conp_fix_args &args, conp_env env, MPI_Comm *world, int me, int nprocs) {
    cutsq0.assign((size_t)(env.ntypes + 1) * (env.ntypes + 1), 0.0);   /* the provider computes no real-space pairs */
    env.cutsq = cutsq0.data();
    fail_if(error, conp_fix_create(&args, &env, &h));
    fail_if(error, install_mpi_comm(h, world, me, nprocs));
  }

  /* km_ewald.cpp:232-275 (re)allocates the provider's tables when the fix's atom counts change; here the handle re-reads the
   * atoms and rebuilds its own index maps (same algorithm as FixConp::post_neighbor :468-539, so the same permanent numbering;
   * results are mapped through TAGS anyway: lib_tag2eleall) */
  void post_neighbor(const conp_atoms &at) {
    /* the handle's hooks want a neighbour list; the provider has no pair work: an empty one (numneigh / first are per-atom arrays) */
    nolist.assign((size_t)at.nlocal + at.nghost + 1, 0);
    conp_neighlist empty;
    empty.inum = 0; empty.ilist = nolist.data(); empty.numneigh = nolist.data(); empty.first = nolist.data();
    empty.neigh = nolist.data(); empty.nneigh = 0;
    fail_if(error, conp_fix_init_list(h, 2, &empty));
    if (first) { fail_if(error, conp_fix_setup_post_neighbor(h, &at)); first = false; }
    else fail_if(error, conp_fix_post_neighbor(h, &at));
    conp_info info;
    fail_if(error, conp_fix_info(h, &info));
    lib_tag2eleall.assign((size_t)info.maxtag_all + 1, 0);
    fail_if(error, conp_fix_get_maps(h, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, lib_tag2eleall.data()));
  }

  template <class Fix> void a_cal(const conp_atoms &at, const Fix *fixconp, double *aaa) {
    const int ne = fixconp->elenum_all, nloc = fixconp->elenum;
    std::vector<double> full((size_t)ne * ne);
    fail_if(error, conp_km_a_cal(h, &at, full.data()));
    /* the library returns each unordered pair folded into the lower triangle; the reference's caller symmetrises afterwards
     * (fix_conp.cpp:826-831), so any single orientation is valid.  Rows / columns go from the library's numbering to the fix's by tag. */
    for (int i = 0; i < nloc; ++i) {
      const size_t li = (size_t)lib_tag2eleall[fixconp->ele2tag[i]];
      for (int j = 0; j < ne; ++j) aaa[(size_t)i * ne + j] += full[li * ne + (size_t)lib_tag2eleall[fixconp->eleall2tag[j]]];
    }
  }

  template <class Fix> void b_cal(const conp_atoms &at, const Fix *fixconp, double *bbb) {
    std::vector<double> ball(fixconp->elenum_all);
    fail_if(error, conp_km_b_cal(h, &at, ball.data()));
    for (int i = 0; i < fixconp->elenum; ++i) bbb[i] = ball[lib_tag2eleall[fixconp->ele2tag[i]]];   /* overwrite (km_ewald.cpp:821) */
  }

  /* 1 for the owned atoms of the group, for *_compute_group_potential */
  const int *group_sel(const int *mask, int nlocal, int groupbit) {
    sel.resize(nlocal);
    for (int i = 0; i < nlocal; ++i) sel[i] = (mask[i] & groupbit) ? 1 : 0;
    return sel.data();
  }

 private:
  LAMMPS_NS::Error *error;
  bool first = true;
  std::vector<int> lib_tag2eleall, nolist, sel;
  std::vector<double> cutsq0;
};

}  // namespace conp_glue
