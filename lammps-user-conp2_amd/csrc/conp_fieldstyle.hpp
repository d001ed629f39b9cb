// struct FieldStyle: `fix efield` with a constant field, optionally coupled to the fix scalar of the same update; struct ObserveStyle:
// the per-group sums of overlapping groups behind the thermo columns (conp_fieldstyle.cpp).
#pragma once
#include "conp_dev.hpp"
#include "conp_kernels.h"

namespace conp {

struct FieldStyle {
  dev::DevCtx &ctx;                                                     // the handle's stream, wait and profiler
  bool have_params = false;
  int nlocal = 0;
  EfieldArgs proto{};                                                   // the constants and tables of set_params
  dev::DevBuf<int> d_sel;
  dev::DevBuf<double> d_part;

  void set_params(const conp_efield_params *p);      // a refused call leaves the handle without a field
  void need_params(const char *who) const {
    if (!have_params) throw dev::ConpError(CONP_ERR_STATE, std::string(who) + " before conp_efield_set_params");
  }
  // d_scalar: the device slot that holds the fix scalar of the last update (couple == 1), or NULL
  void post_force(const double *d_x, const double *d_q, const int *d_image, double *d_f, const double *e, const double *d_scalar,
                  double couple_scale, double *d_out, double *d_vatom);
};

struct ObserveStyle {
  dev::DevCtx &ctx;
  bool have_params = false;
  int nlocal = 0, ngroups = 0;
  ObserveArgs proto{};
  dev::DevBuf<int> d_type, d_mask;
  dev::DevBuf<double> d_mass, d_part;

  void set_params(const conp_observe_params *p);     // a refused call leaves the handle without groups
  void need_params(const char *who) const {
    if (!have_params) throw dev::ConpError(CONP_ERR_STATE, std::string(who) + " before conp_observe_set_params");
  }
  void observe(const double *d_x, const double *d_q, const double *d_v, const int *d_image, double *d_out);
};

}  // namespace conp
