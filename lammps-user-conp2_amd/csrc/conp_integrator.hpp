// struct Integrator: velocity Verlet with a Nose-Hoover chain per thermostatted group (conp_integrator.cpp).
#pragma once
#include "conp_dev.hpp"
#include "conp_kernels.h"

namespace conp {

struct Integrator {
  dev::DevCtx &ctx;                                                     // the handle's stream, wait and profiler
  bool have_params = false, is_setup = false, any_nvt = false;
  int nlocal = 0, ngroups = 0;
  int cur = 0;                                                          // which half of d_state holds the chains: `initial` flips it
  IntegrateArgs proto{};                                                // the constants and tables of set_params
  dev::DevBuf<int> d_type, d_group;
  dev::DevBuf<double> d_mass, d_state, d_part, d_factor, d_raw;
  std::vector<double> raw_h;

  void set_params(const conp_integrate_params *p);   // a refused call leaves the handle without an integrator
  void need_params(const char *who) const {
    if (!have_params) throw dev::ConpError(CONP_ERR_STATE, std::string(who) + " before conp_integrate_set_params");
  }
  void need_setup(const char *who) const {
    need_params(who);
    if (any_nvt && !is_setup) throw dev::ConpError(CONP_ERR_STATE, std::string(who) + " before conp_integrate_setup_device");
  }
  double *state(int half) { return d_state.p + (size_t)half * INTEGRATE_G * INTEGRATE_STATE_W; }
  IntegrateArgs args(const double *t_target, const char *who) const;     // proto with the checked targets
  void setup(const double *d_v, const double *t_target);
  void initial(double *d_x, double *d_v, const double *d_f, const double *t_target);
  void final_(double *d_v, const double *d_f, double *d_out);
  void temperature(const double *d_v, double *d_out);
  void get_state(double *state8);
  void set_state(const double *state8);
};

}  // namespace conp
