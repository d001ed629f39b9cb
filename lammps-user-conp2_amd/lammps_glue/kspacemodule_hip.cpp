#include "kspacemodule_hip.h"

#ifndef CONP_GLUE_MOCK
#include "fix_conp.h"
#endif

using namespace LAMMPS_NS;
using conp_glue::fail_if;

KSpaceModuleHip::KSpaceModuleHip(LAMMPS *lmp) : KSpaceModule(), Pointers(lmp), ph(error) {}

conp_atoms KSpaceModuleHip::view() {
  return av.flat(atom, [this](int i) { return fixconp->electrode_check(i); });   // fix_conp.cpp:599-605, through the registered fix
}

/* km_ewald.cpp:63-132.  The fix was registered just before (fix_conp.cpp:409), so its public members are readable here. */
void KSpaceModuleHip::conp_setup(bool lowmem) {
  lowmemflag = lowmem;           /* phases are regenerated on the fly: no csk/snk[Ne][K] table choice to make (km_ewald.cpp:261-268) */
  if (fixconp == nullptr) error->all(FLERR, "KSpaceModuleHip: register_fix() must precede conp_setup()");
  if (ph.h == nullptr) {
    conp_fix_args fa = conp_glue::provider_args(0);
    fa.eta = fixconp->eta; fa.lowmem = lowmem ? 1 : 0;
    ph.create(fa, conp_glue::base_env(force, domain, atom, comm, world, force->kspace), &world, comm->me, comm->nprocs);
  }
  double qsqsum = 0.0;                                        /* km_ewald.cpp:72-78 */
  for (int i = 0; i < atom->nlocal; i++) qsqsum += atom->q[i] * atom->q[i];
  MPI_Allreduce(MPI_IN_PLACE, &qsqsum, 1, MPI_DOUBLE, MPI_SUM, world);
  fail_if(error, conp_km_conp_setup(ph.h, qsqsum, (int64_t)atom->natoms));
}

void KSpaceModuleHip::conp_post_neighbor(bool, bool) { ph.post_neighbor(view()); }

void KSpaceModuleHip::a_cal(double *aaa) { ph.a_cal(view(), fixconp, aaa); }

void KSpaceModuleHip::b_cal(double *bbb) { ph.b_cal(view(), fixconp, bbb); }

/* the exact Ewald potentials of the owned atoms (conp_ewald_*): g_i for the group, u_i = g_i + 2 g_ewald q_i / sqrt(pi) per atom.
 * compute_particle_potential is rank-local like PPPMConpHip's: under several ranks a call without a collective entry since the last
 * update is error->one, not a hidden collective. */
double KSpaceModuleHip::compute_particle_potential(int i) {
  conp_atoms at = view();
  double u = 0.0;
  if (conp_ewald_compute_particle_potential(ph.h, &at, i, &u) != CONP_OK) error->one(FLERR, conp_last_error());
  return u;
}

void KSpaceModuleHip::compute_group_potential(int groupbit, double *recv) {
  conp_atoms at = view();
  fail_if(error, conp_ewald_compute_group_potential(ph.h, &at, ph.group_sel(atom->mask, atom->nlocal, groupbit), recv));
}
