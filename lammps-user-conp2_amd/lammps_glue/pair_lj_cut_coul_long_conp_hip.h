/* PairLJCutCoulLongConpHip -- `pair_style lj/cut/coul/long/conp/hip`: the real-space pair loop of an MD step with a constant-
 * potential fix, on the device.  The class is LAMMPS' PairLJCutCoulLong with compute(eflag, vflag) replaced:
 * settings, pair_coeff, mixing, init_one and extract stay the base class's, so an input script changes the style's name only.
 * compute() hands atom->x / q / f to conp_pair_compute on the handle a conp/hip (conq/hip, cond/hip) fix already owns -- or that of
 * the KSpaceModuleHip provider of the reference's fix conp -- found through Modify::fix like `kspace_style ewald/conp/hip` does:
 *   conp_pair_set_params   once, from the base class's lj1..lj4, offset, cut_ljsq, cutsq, cut_coul and force->special_lj / special_coul;
 *                          the tables are looked at again on every re-neighbouring step and sent again if pair_coeff changed them
 *   conp_pair_set_list     whenever the neighbour list has been rebuilt (neighbor->ago == 0), from the style's own half list
 *   conp_pair_compute      every step; eng_vdwl, eng_coul, virial, eatom and vatom are filled according to the flags
 * The virial is the pair tally (no_virial_fdotr = 1).  Ghost entries of f, eatom and vatom are what LAMMPS' reverse communication
 * folds back, as with the base class.  Not supported: Coulomb tables -- compute() stops unless `pair_modify table 0` is set. */
#ifdef PAIR_CLASS

PairStyle(lj/cut/coul/long/conp/hip,PairLJCutCoulLongConpHip)

#else

#ifndef LMP_PAIR_LJ_CUT_COUL_LONG_CONP_HIP_H
#define LMP_PAIR_LJ_CUT_COUL_LONG_CONP_HIP_H

#include "conp_glue_common.h"
#include "fix_conp_hip.h"
#include "kspacemodule_hip.h"
#ifndef CONP_GLUE_MOCK
#include "pair_lj_cut_coul_long.h"
#endif

namespace LAMMPS_NS {

class PairLJCutCoulLongConpHip : public PairLJCutCoulLong {
 public:
  explicit PairLJCutCoulLongConpHip(class LAMMPS *);
  void compute(int eflag, int vflag) override;
  conp_fix *handle() { return handle_; }
  int list_uploads() const { return n_list_uploads; }    /* how often conp_pair_set_list ran */

 private:
  conp_fix *handle_ = nullptr;       /* owned by the fix (or its provider) */
  FixConpHip *fixhip = nullptr;
  FixConp *fixconp = nullptr;
  conp_glue::AtomView av;
  bool params_set = false, list_set = false;
  int n_list_uploads = 0;
  std::vector<int> first_flat, neigh_flat;
  std::vector<double> tables, tables_sent;       /* the seven tables flattened, cut_coul, the special factors */
  void flatten_tables();
  void find_handle();
  void send_params();
  void send_list();
};

}  // namespace LAMMPS_NS
#endif
#endif
