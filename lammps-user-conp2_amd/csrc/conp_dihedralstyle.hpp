// struct DihedralStyle: opls / harmonic dihedral and harmonic / cvff improper forces over the caller's topology lists
// (conp_dihedralstyle.cpp).
#pragma once
#include "conp_dev.hpp"
#include "conp_kernels.h"

namespace conp {

struct DihedralStyle {
  dev::DevCtx &ctx;                                                     // the handle's stream, wait and profiler
  bool have_params = false, have_lists = false;
  int dstyle = 0, istyle = 0, ndihedraltypes = 0, nimpropertypes = 0, newton_bond = 0;
  int nlocal = 0, nall = 0, ndihedral = 0, nimproper = 0;
  double prd[3] = {0.0, 0.0, 0.0};
  dev::DevBuf<double> d_dcoef, d_icoef, d_term, d_part, d_x, d_f, d_ev, d_ea, d_va;
  dev::DevBuf<int> d_dihedral, d_improper, d_slot_ptr, d_slot;
  std::vector<double> out_h;

  void set_params(const conp_dihedral_params *p);    // drops the lists: they were checked against the old tables
  void set_lists(const conp_dihedral_lists *l);
  void need_ready(const char *who) const {
    if (!have_params) throw dev::ConpError(CONP_ERR_STATE, std::string(who) + " before conp_dihedral_set_params");
    if (!have_lists) throw dev::ConpError(CONP_ERR_STATE, std::string(who) + " before conp_dihedral_set_lists");
  }
  void enqueue(const double *dx, double *df, double *dev, double *dea, double *dva);
  // stages at->x, downloads and adds into f, overwrites the rest
  void compute_host(const conp_atoms *at, double *f, double *eng, double *vir, double *eatom, double *vatom);
};

}  // namespace conp
