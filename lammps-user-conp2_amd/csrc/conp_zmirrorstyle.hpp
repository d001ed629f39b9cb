// struct ZmirrorStyle: `fix zmirror` -- the receiving group kept as the z mirror image of the sending group (conp_zmirrorstyle.cpp,
// DESIGN.md section 25).
#pragma once
#include <vector>

#include "conp_dev.hpp"
#include "conp_kernels.h"

namespace conp {

struct ZmirrorStyle {
  dev::DevCtx &ctx;                                                     // the handle's stream, wait and profiler
  bool have_params = false;
  int npairs = 0, nevery = 1;
  double zoffset = 0.0;                                                 // 2 boxlo_z + zprd
  std::vector<int> src_h, dst_h;                                        // the map, in ascending source index
  dev::DevBuf<int2> d_map;                                              // (source, target) per pair

  void set_params(const conp_zmirror_params *p);     // a refused call leaves the handle without a mirror
  void need_params(const char *who) const {
    if (!have_params) throw dev::ConpError(CONP_ERR_STATE, std::string(who) + " before conp_zmirror_set_params");
  }
  void post_integrate(double *d_x, long long ntimestep);
};

}  // namespace conp
