#include "pppm_conp_hip.h"

#include <cstring>

#ifndef CONP_GLUE_MOCK
#include "domain.h"
#include "fix_conp.h"
#include "modify.h"
#endif

using namespace LAMMPS_NS;
using conp_glue::fail_if;

/* unlike the Ewald provider, the fix does not delete force->kspace (fix_conp.cpp:207): the handle goes with the style */
PPPMConpHip::PPPMConpHip(LAMMPS *lmp) : PPPM(lmp), KSpaceModule(), ph(error) {}

conp_atoms PPPMConpHip::view() {
  return av.flat(atom, [this](int i) { return fixconp ? fixconp->electrode_check(i) : 0; });
}

void PPPMConpHip::conp_setup(bool lowmem) {
  lowmemflag = lowmem;
  if (fixconp == nullptr) error->all(FLERR, "pppm/conp/hip: register_fix() must precede conp_setup()");
  /* several MPI ranks: the mesh is not sharded -- rank 0 owns it; the ranks' charged electrolyte atoms are gathered per update
   * like for the Ewald provider, the electrode vector is summed over the ranks (pppm_conp.cpp:114,122 shard the mesh instead) */
  if (ph.h == nullptr) {
    conp_fix_args fa = conp_glue::provider_args(1);
    fa.eta = fixconp->eta; fa.lowmem = lowmem ? 1 : 0;
    conp_env env = conp_glue::base_env(force, domain, atom, comm, world, this);                                      /* own KSpace members */
    env.pppm_nx = nx_pppm; env.pppm_ny = ny_pppm; env.pppm_nz = nz_pppm; env.pppm_order = order;                      /* PPPM::set_grid_global's result */
    ph.create(fa, env, &world, comm->me, comm->nprocs);
  }
}

void PPPMConpHip::conp_post_neighbor(bool, bool) { ph.post_neighbor(view()); }

/* the Ewald matrix, like PPPMCONP::a_cal's temporary KSpaceModuleEwald (:91-101) */
void PPPMConpHip::a_cal(double *aaa) { ph.a_cal(view(), fixconp, aaa); }

void PPPMConpHip::conp_pre_force() {           /* pppm_conp.h:42: elyte_mapped = false -- a new step, the kept brick is stale */
  if (ph.h) fail_if(error, conp_pppm_keep_density(ph.h, 1));
}

void PPPMConpHip::b_cal(double *bbb) {          /* spread, Poisson solve, stencil gather on the device mesh (:269-316) */
  if (!bcal_done) fail_if(error, conp_pppm_keep_density(ph.h, 1));      /* the make_rho override wants the electrolyte brick of every b_cal */
  bcal_done = true;
  ph.b_cal(view(), fixconp, bbb);
}

void PPPMConpHip::particle_map() {              /* pppm_conp.cpp:428-432 */
  if (!bcal_done || fixconp == nullptr) PPPM::particle_map();
  /* else: the library maps the atoms on the device when it spreads them (elyte_particle_map :126-170 inside b_cal) */
}

void PPPMConpHip::make_rho() {                  /* pppm_conp.cpp:434-450 */
  if (!bcal_done || fixconp == nullptr) { PPPM::make_rho(); return; }
  conp_atoms at = view();
  dens.resize((size_t)nx_pppm * ny_pppm * nz_pppm);
  /* electrolyte brick as b_cal left it (not spread again on one rank) + the electrode brick of the CURRENT charges (ele_make_rho
   * :385-426); the library's bricks are [nz][ny][nx] with the ghost planes folded in, so the owned points are filled and the
   * ghost planes left zero: PPPM::compute's ghost sum (gc->reverse_comm) then adds nothing */
  fail_if(error, conp_pppm_make_rho(ph.h, &at, dens.data(), nullptr, nullptr));
  std::memset(&(density_brick[nzlo_out][nylo_out][nxlo_out]), 0, (size_t)ngrid * sizeof(FFT_SCALAR));
  for (int iz = nzlo_in; iz <= nzhi_in; ++iz)
    for (int iy = nylo_in; iy <= nyhi_in; ++iy)
      for (int ix = nxlo_in; ix <= nxhi_in; ++ix)
        density_brick[iz][iy][ix] = (FFT_SCALAR)dens[((size_t)iz * ny_pppm + iy) * nx_pppm + ix];
}

double PPPMConpHip::compute_particle_potential(int i) {
  // RANK-LOCAL, like the reference's (pppm_conp.cpp:452-485; compute_potential_atom.cpp:168-174 calls it once per owned atom of
  // the group -- a different number of calls on every rank): a stencil gather from the mesh potential the library cached when a
  // collective entry last formed it (compute_group_potential, compute potential/atom).  Under several ranks a call without such
  // a brick is an error (error->one: only this rank is here), not a hidden collective.
  conp_atoms at = view();
  double u = 0.0;
  if (conp_pppm_compute_particle_potential(ph.h, &at, i, &u) != CONP_OK) error->one(FLERR, conp_last_error());
  return u;
}

void PPPMConpHip::compute_group_potential(int groupbit, double *recv) {
  conp_atoms at = view();
  fail_if(error, conp_pppm_compute_group_potential(ph.h, &at, ph.group_sel(atom->mask, atom->nlocal, groupbit), recv));
}

void PPPMConpHip::total_density(double *density_brick) {
  conp_atoms at = view();
  fail_if(error, conp_pppm_make_rho(ph.h, &at, density_brick, nullptr, nullptr));
}

/* kspace_style pppm/conp/hip ACCURACY [device] -- the optional second word selects the device compute() */
void PPPMConpHip::settings(int narg, char **arg) {
  if (narg == 2) {
    if (std::strcmp(arg[1], "device") != 0) error->all(FLERR, "Illegal kspace_style pppm/conp/hip command: the optional second word is `device`");
    device_mode = true;
    narg = 1;
  }
  PPPM::settings(narg, arg);
}

/* the handle compute() runs on: the style's own (the reference's fix conp registered and b_cal has created it), else that of a
 * conp/hip fix (found through Modify::fix like `compute potential/atom/hip` and ewald/conp/hip do); the library refuses a handle
 * without the `pppm` keyword */
conp_fix *PPPMConpHip::force_handle() {
  if (ph.h != nullptr) return ph.h;
  for (int f = 0; f < modify->nfix; ++f)
    if (auto *fh = dynamic_cast<FixConpHip *>(modify->fix[f]))
      if (fh->handle() != nullptr) { fixhip = fh; return fh->handle(); }
  fixhip = nullptr;
  return nullptr;
}

void PPPMConpHip::compute(int eflag, int vflag) {
  if (!device_mode) { PPPM::compute(eflag, vflag); return; }
  ev_init(eflag, vflag);
  if (vflag_atom) error->all(FLERR, "kspace_style pppm/conp/hip device does not tally a per-atom virial");
  if (domain->triclinic) error->all(FLERR, "kspace_style pppm/conp/hip device does not support a triclinic box");
  if (differentiation_flag != 0) error->all(FLERR, "kspace_style pppm/conp/hip device supports kspace_modify diff ik only");
  conp_fix *h = force_handle();
  if (h == nullptr)
    error->all(FLERR, "kspace_style pppm/conp/hip device needs a fix with the pppm keyword: a conp/hip fix, or fix conp after its first b_cal");
  conp_atoms at = av.flat(atom, [this](int i) { return fixconp ? fixconp->electrode_check(i) : (fixhip ? fixhip->electrode_check(i) : 0); });
  /* atom->f is one contiguous [nmax][3] block behind the row pointers (Memory::create): accumulated in place.  The entry spreads the
   * atoms it is given on every call, so steps on which the fix skips its update get the forces of the moved atoms */
  double *f = atom->nlocal ? &atom->f[0][0] : nullptr;
  fail_if(error, conp_pppm_compute_forces(h, &at, f, eflag_global ? &energy : nullptr, vflag_global ? virial : nullptr,
                                          eflag_atom ? eatom : nullptr));
}
