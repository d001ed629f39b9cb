// struct PotentialAtom: `compute potential/atom` on the device -- the scratch of conp_potential_atom_device and its two launches
// around the k-space provider's part (conp_potatomstyle.cpp, conp_potatom.hip).
#pragma once
#include "conp_dev.hpp"
#include "conp_kernels.h"
#include "conp_kspace_common.hpp"

namespace conp {

struct PotentialAtom {
  dev::DevCtx &ctx;                                                     // the handle's stream, wait and profiler
  dev::DevBuf<double> d_u;                // [nlocal] the k-space potential u_i of the targets, by owned index
  dev::DevBuf<double> d_kf_sums;          // Q, Q2, M, M2 of the call's owned atoms with the workgroups' partial rows behind them

  // d_pot[0, ntotal): the pair part of the selected rows (section 26's order), 0.0 on the others
  void pair_part(const PotPairArgs &a, const TransposedView &tv);
  // d_u sized for nlocal owned atoms: where the provider writes u
  double *u_buffer(int nlocal) { d_u.reserve(nlocal); return d_u.p; }
  // the host entry's tail on the targets; under slab the four sums of the nlocal owned atoms (a.x, a.q) are formed first
  void finish(PotFinishArgs a, int nlocal);
};

}  // namespace conp
