/* KSpaceModuleHip -- the Ewald k-space provider of USER-CONP2 (km_ewald.h:27-80) served by libconp_hip.so.
 * It IS a KSpaceModule of the reference (kspacemodule.h:26-45): a maintainer who keeps the reference's FixConp replaces
 *     else kspmod = new KSpaceModuleEwald(lmp);          (fix_conp.cpp:408)
 * by  else kspmod = new KSpaceModuleHip(lmp);
 * and nothing else -- `kspmod->register_fix(this)` (:409) hands the fix over, and the provider reads the fix's public members
 * (elenum, elenum_all, ele2tag, eleall2tag, eta, electrode_check(): fix_conp.h:58-89) exactly as KSpaceModuleEwald does.
 * Ownership: the provider creates its own conp_fix handle in conp_setup() and destroys it in its destructor; FixConp deletes its
 * Ewald provider in ~FixConp (fix_conp.cpp:207), so the handle's life is the fix's.  FixConpHip (fix_conp_hip.h) replaces the
 * whole fix instead and does not use this class. */
#ifndef LMP_FIXCONP_KM_HIP_H
#define LMP_FIXCONP_KM_HIP_H

#include "conp_glue_common.h"
#ifdef CONP_GLUE_MOCK
#include "mock_lammps/conp2_mock.h"
#else
#include "kspacemodule.h" /* the reference's header: KSpaceModule, FixConp */
#include "pointers.h"
#endif

namespace LAMMPS_NS {

class KSpaceModuleHip : public KSpaceModule, protected Pointers {
 public:
  explicit KSpaceModuleHip(LAMMPS *lmp);
  void conp_setup(bool lowmem) override;                 /* km_ewald.cpp:63-132: handle creation + k tables */
  void conp_post_neighbor(bool, bool) override;          /* km_ewald.cpp:232-275: the handle follows the fix's atoms */
  void a_cal(double *aaa) override;                      /* km_ewald.cpp:147-151 : aaa[elenum][elenum_all] +=, k-space part */
  void a_read() override {}                              /* km_ewald.cpp:134-145: the phase tables are built inside a_cal / b_cal */
  void b_cal(double *bbb) override;                      /* km_ewald.cpp:153-167 : bbb[elenum] =, local electrode order */
  /* The reference's KSpaceModuleEwald returns 0 for both potentials (kspacemodule.h:38-39); here they are the exact Ewald sums
   * (conp_ewald_*, include/conp_hip.h), so that compute potential/atom works without a mesh.  update_charge, conp_pre_force and
   * return_qsum keep the base-class defaults. */
  double compute_particle_potential(int i) override;                  /* rank-local, from the cached structure factor */
  void compute_group_potential(int groupbit, double *recv) override;  /* collective */
  conp_fix *handle() { return ph.h; }

 private:
  conp_glue::ProviderHandle ph;      /* destroys the handle with the provider */
  conp_glue::AtomView av;
  conp_atoms view();
};

}  // namespace LAMMPS_NS
#endif
