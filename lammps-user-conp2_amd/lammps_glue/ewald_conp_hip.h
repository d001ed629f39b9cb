/* EwaldConpHip -- `kspace_style ewald/conp/hip`: the reciprocal-space forces, energy and virial of an MD step with a constant-
 * potential fix, on the device.  After the fix's pre_force has written the electrode charges LAMMPS calls force->kspace->compute():
 * this style hands atom->x / q / f to conp_ewald_compute_forces_vatom on the handle the fix already owns -- the same k list, the same
 * structure-factor machinery as the charge update -- instead of LAMMPS' own Ewald::compute on the CPU.
 * The handle is that of a conp/hip (conq/hip, cond/hip) fix, or of the KSpaceModuleHip provider of the reference's fix conp, found
 * through Modify::fix like `compute potential/atom/hip` does.  A handle whose provider is the mesh refuses (CONP_ERR_STATE).
 * compute() forms the structure factor of the atoms it is given on every call (conp_ewald_compute), whether or not the fix updated
 * the charges on that step.
 * Input script: `kspace_style ewald/conp/hip ACCURACY` together with `kspace_modify gewald G` -- the style does not estimate g_ewald
 * from the accuracy (init() stops without one); `kspace_modify slab` and `force` act through the base class as usual.  The
 * per-atom virial (`compute stress/atom`, vflag_atom) is tallied into vatom on the device.  Not supported:
 * triclinic boxes (init() stops with an error). */
#ifdef KSPACE_CLASS

KSpaceStyle(ewald/conp/hip,EwaldConpHip)

#else

#ifndef LMP_EWALD_CONP_HIP_H
#define LMP_EWALD_CONP_HIP_H

#include "conp_glue_common.h"
#include "fix_conp_hip.h"
#include "kspacemodule_hip.h"

namespace LAMMPS_NS {

class EwaldConpHip : public KSpace {
 public:
  explicit EwaldConpHip(class LAMMPS *);
  void settings(int, char **) override;
  void init() override;
  void setup() override {}
  void compute(int eflag, int vflag) override;
  conp_fix *handle() { return handle_; }

 private:
  conp_fix *handle_ = nullptr;       /* owned by the fix (or its provider) */
  FixConpHip *fixhip = nullptr;
  FixConp *fixconp = nullptr;
  conp_glue::AtomView av;
  void find_handle();
};

}  // namespace LAMMPS_NS
#endif
#endif
