// struct ShakeStyle: SHAKE bond and angle constraints of small clusters (conp_shakestyle.cpp).
#pragma once
#include "conp_dev.hpp"
#include "conp_kernels.h"

namespace conp {

struct ShakeStyle {
  dev::DevCtx &ctx;                                                     // the handle's stream, wait and profiler
  bool have_params = false;
  int nlocal = 0, ncluster = 0;
  double dt = 0.0, ftm2v = 0.0;
  ShakeArgs proto{};                                                    // the constants and tables of set_params
  dev::DevBuf<int> d_type, d_cluster, d_member;
  dev::DevBuf<double> d_mass, d_bond_d, d_angle_d, d_part;

  void set_params(const conp_shake_params *p);       // a refused call leaves the handle without constraints
  void need_params(const char *who) const {
    if (!have_params) throw dev::ConpError(CONP_ERR_STATE, std::string(who) + " before conp_shake_set_params");
  }
  void correct(double *d_x);
  // post_force: dtfsq = dt dt ftm2v; setup: half of it and no d_vatom
  void force(const double *d_x, const double *d_v, double *d_f, double *d_out, double *d_vatom, bool setup);
  void check(const double *d_x, double *d_out);
};

}  // namespace conp
