/* ComputePotentialAtomHip -- `compute ID group potential/atom/hip [pair] [kspace] [noqsum] [eta ETA molL molR]`: the reference's
 * `compute potential/atom` (compute_potential_atom.h:16, compute_potential_atom.cpp:49-345) with its pair loop, mesh gather and
 * slab correction done by libconp_hip.so in one call (conp_compute_potential_atom).  Same arguments, same errors, same output
 * (per-atom vector in volts).  The k-space part comes from `kspace_style pppm/conp/hip` (the mesh, as the reference needs a
 * "compatible KSpace provider like pppm/conp", :110) or, without it, from the exact Ewald sums of the handle of a `conp/hip`
 * (`conq/hip`, `cond/hip`) fix or of the reference's fix conp with the KSpaceModuleHip provider. */
#ifdef COMPUTE_CLASS

ComputeStyle(potential/atom/hip,ComputePotentialAtomHip)

#else

#ifndef LMP_COMPUTE_POTENTIAL_ATOM_HIP_H
#define LMP_COMPUTE_POTENTIAL_ATOM_HIP_H

#include "conp_glue_common.h"
#ifdef CONP_GLUE_MOCK
#include "mock_lammps/conp2_mock.h"
#else
#include "compute.h"
#endif

namespace LAMMPS_NS {

class ComputePotentialAtomHip : public Compute {
 public:
  ComputePotentialAtomHip(class LAMMPS *, int, char **);
  ~ComputePotentialAtomHip() override;
  void init() override {}
  void setup() override;
  void compute_peratom() override;
  double memory_usage() override;

 private:
  class PPPMConpHip *provider;
  conp_fix *handle_;                 /* the handle the per-atom call runs on: the pppm style's, or an Ewald one */
  class FixConp *fixconp;            /* electrode_check: the reference's fix (pppm/conp/hip, KSpaceModuleHip) ... */
  class FixConpHip *fixhip;          /* ... or the conp/hip fix */
  bool pairflag, kspaceflag, etaflag, qsumflag;
  int nmax, molidL, molidR;
  double eta;
  double *potential;
  conp_glue::AtomView av;
  std::vector<int> sel, etasel, first, neigh;
  std::vector<double> out;
};

}  // namespace LAMMPS_NS
#endif
#endif
