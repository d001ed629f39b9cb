// struct GhostMap: ghost atoms built, updated and folded back on the device (conp_ghostmap.cpp).
#pragma once
#include "conp_dev.hpp"
#include "conp_kernels.h"

namespace conp {

struct GhostMap {
  dev::DevCtx &ctx;
  bool built = false;
  int nlocal = 0, nghost = 0;
  double prd[3] = {0.0, 0.0, 0.0};
  dev::DevBuf<int> d_shift, d_count, d_start, d_nimg, d_ofirst, d_owner, d_img, d_list;
  dev::DevBuf<long long> d_total;
  static constexpr int MAX_SHIFTS = 4096;

  void build(const double *dx, const conp_ghost_build_args *a, int *nghost_out);
  void need_built(const char *who) const {
    if (!built) throw dev::ConpError(CONP_ERR_STATE, std::string(who) + " before a successful conp_ghost_build_device");
  }
  void fill(double *dx, double *dq);
  void fill_int(int *dv, int width);
  void fold(double *dv, int width);
  void get(int *nlocal_out, int *nghost_out, int *owner, int *img);
};

void atoms_wrap(dev::DevCtx &ctx, double *dx, int nlocal_, const double *boxlo, const double *boxhi, const int *periodic, int *dimage);

}  // namespace conp
