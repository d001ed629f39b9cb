#include "ewald_conp_hip.h"

#include <cmath>

#ifndef CONP_GLUE_MOCK
#include "fix_conp.h"
#include "modify.h"
#endif

using namespace LAMMPS_NS;
using conp_glue::fail_if;

EwaldConpHip::EwaldConpHip(LAMMPS *lmp) : KSpace(lmp) {}

/* kspace_style ewald/conp/hip ACCURACY -- the relative accuracy, as for LAMMPS' own ewald */
void EwaldConpHip::settings(int narg, char **arg) {
  if (narg != 1) error->all(FLERR, "Illegal kspace_style ewald/conp/hip command");
  accuracy_relative = std::fabs(utils::numeric(FLERR, arg[0], false, lmp));
}

/* `accuracy` in force units as Ewald::init forms it; g_ewald is NOT estimated from it here: the fix (FixConpHip::init, conp_env) and
 * the coul/long pair style read force->kspace->g_ewald, so it has to come from `kspace_modify gewald`.  Orthogonal boxes only.
 * The fix creates its handle in its own init / setup, after this one: the lookup is repeated at the first compute(). */
void EwaldConpHip::init() {
  if (domain->triclinic) error->all(FLERR, "kspace_style ewald/conp/hip does not support a triclinic box");
  if (g_ewald <= 0.0)
    error->all(FLERR, "kspace_style ewald/conp/hip does not estimate the Ewald parameter: set it with kspace_modify gewald");
  accuracy = accuracy_absolute >= 0.0 ? accuracy_absolute : accuracy_relative * two_charge_force;
  if (accuracy <= 0.0) error->all(FLERR, "kspace_style ewald/conp/hip needs a positive accuracy");
  find_handle();
}

void EwaldConpHip::find_handle() {
  handle_ = nullptr; fixhip = nullptr; fixconp = nullptr;
  for (int f = 0; f < modify->nfix && handle_ == nullptr; ++f) {
    if (auto *fh = dynamic_cast<FixConpHip *>(modify->fix[f])) {
      if (fh->handle() != nullptr) { fixhip = fh; handle_ = fh->handle(); }
    } else if (auto *fc = dynamic_cast<FixConp *>(modify->fix[f])) {
      auto *km = dynamic_cast<KSpaceModuleHip *>(fc->kspmod);
      if (km != nullptr && km->handle() != nullptr) { fixconp = fc; handle_ = km->handle(); }
    }
  }
}

void EwaldConpHip::compute(int eflag, int vflag) {
  ev_init(eflag, vflag);
  if (handle_ == nullptr) find_handle();
  if (handle_ == nullptr) error->all(FLERR, "kspace_style ewald/conp/hip needs a conp/hip fix (or fix conp with the hip provider)");
  conp_atoms at = av.flat(atom, [this](int i) { return fixconp ? fixconp->electrode_check(i) : fixhip->electrode_check(i); });
  /* atom->f is one contiguous [nmax][3] block behind the row pointers (Memory::create): accumulated in place */
  double *f = atom->nlocal ? &atom->f[0][0] : nullptr;
  /* S of the atoms as they are NOW, every call: conp_ewald_compute_forces alone would reuse the S a collective entry cached since
   * the fix's last update, and the atoms move between updates (fix ... N with N > 1, the reference fix's skipped b_cal, minimize,
   * a second run).  When the fix did update this step nothing is cached yet, so this is the formation the entry would do itself. */
  fail_if(error, conp_ewald_compute(handle_, &at));
  /* vatom is one contiguous [nmax][6] block behind its row pointers, like atom->f; its owned rows are overwritten (Ewald::compute's
   * per-atom virial; with vatom NULL the entry is conp_ewald_compute_forces bit for bit) */
  fail_if(error, conp_ewald_compute_forces_vatom(handle_, &at, f, eflag_global ? &energy : nullptr, vflag_global ? virial : nullptr,
                                                 eflag_atom ? eatom : nullptr, vflag_atom && atom->nlocal ? &vatom[0][0] : nullptr));
}
