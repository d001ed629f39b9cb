// Ghost atoms on the device (conp_ghost.hip): Comm::borders / forward_comm / reverse_comm of one rank.
// The build keeps owner and image of every ghost and, per owner, the ascending list of its ghosts; fill, fill_int and fold only
// enqueue.  Separate from map_ghosts / ghost_mode of the host-array path (conp_env.ghost_images).
#include "conp_ghostmap.hpp"

#include <cmath>

namespace conp {
using namespace dev;

void GhostMap::build(const double *dx, const conp_ghost_build_args *a, int *nghost_out) {
  built = false;                          // a build that is refused leaves the handle without ghosts
  if (!a || !nghost_out) throw ConpError(CONP_ERR_ARG, "null argument");
  if (a->nlocal < 0) throw ConpError(CONP_ERR_ARG, "conp_ghost_build_device: negative nlocal");
  if (!dx && a->nlocal > 0) throw ConpError(CONP_ERR_ARG, "conp_ghost_build_device: d_x is NULL");
  if (!(a->cutghost >= 0.0)) throw ConpError(CONP_ERR_ARG, "conp_ghost_build_device: cutghost is negative or not a number");
  GhostBuildArgs g;
  double nshift_d = 1.0;
  int m[3];
  for (int c = 0; c < 3; ++c) {
    if (!std::isfinite(a->boxlo[c]) || !std::isfinite(a->boxhi[c]))
      throw ConpError(CONP_ERR_ARG, "conp_ghost_build_device: a box bound is not finite");
    if (a->periodic[c] && !(a->boxhi[c] > a->boxlo[c]))
      throw ConpError(CONP_ERR_ARG, "conp_ghost_build_device: boxhi <= boxlo in a periodic dimension");
    g.prd[c] = a->boxhi[c] - a->boxlo[c];
    g.lo[c] = a->boxlo[c] - a->cutghost;
    g.hi[c] = a->boxhi[c] + a->cutghost;
    const double mc = a->periodic[c] ? std::ceil(a->cutghost / g.prd[c]) : 0.0;
    nshift_d *= 2.0 * mc + 1.0;
    if (!(nshift_d - 1.0 <= (double)MAX_SHIFTS)) throw ConpError(CONP_ERR_ARG, "conp_ghost_build_device: more than 4096 shifts");
    m[c] = (int)mc;
  }
  if (a->nlocal >= (1 << 30)) throw ConpError(CONP_ERR_NUMERIC, "conp_ghost_build_device: 2^30 atoms or more (neighbour entries keep 30 bits)");
  std::vector<int> shifts;
  for (int sx = -m[0]; sx <= m[0]; ++sx)
    for (int sy = -m[1]; sy <= m[1]; ++sy)
      for (int sz = -m[2]; sz <= m[2]; ++sz)
        if (sx || sy || sz) { shifts.push_back(sx); shifts.push_back(sy); shifts.push_back(sz); }
  const int nl = a->nlocal, nshift = (int)(shifts.size() / 3), nblock = (nl + 63) / 64;
  const size_t ncount = (size_t)nshift * nblock;
  if (ncount >= (1ull << 31))                   // (the scan takes an int length; 2^37 image tests would be behind this)
    throw ConpError(CONP_ERR_NUMERIC, "conp_ghost_build_device: shifts times blocks of 64 owners reach 2^31");
  ctx.sync();                                      // no kernel may be reading the old map
  long long total = 0;
  if (ncount > 0) {
    d_shift.upload(shifts, ctx.stream);
    d_count.reserve(ncount); d_start.reserve(ncount);
    d_nimg.reserve((size_t)nl); d_ofirst.reserve((size_t)nl);
    d_total.reserve(1);
    g.nlocal = nl; g.nblock = nblock; g.nshift = nshift; g.x = dx; g.shift = d_shift.p;
    g.count = d_count.p; g.nimg = d_nimg.p; g.start = nullptr; g.ofirst = nullptr;
    g.nghost = 0; g.owner = nullptr; g.img = nullptr; g.list = nullptr;
    launch_ghost_images(ctx.stream, g, false);
    launch_neigh_scan(ctx.stream, nl, d_nimg.p, d_ofirst.p, d_total.p);
    launch_neigh_scan(ctx.stream, (int)ncount, d_count.p, d_start.p, d_total.p);
    HIP_TRY(hipMemcpyAsync(&total, d_total.p, sizeof total, hipMemcpyDeviceToHost, ctx.stream));
    HIP_TRY(hipGetLastError());
    ctx.sync();
    if ((long long)nl + total >= (1ll << 30))
      throw ConpError(CONP_ERR_NUMERIC, "conp_ghost_build_device: nlocal + nghost reaches 2^30 (neighbour entries keep 30 bits)");
    if (total > 0) {
      d_owner.reserve((size_t)total); d_img.reserve((size_t)total * 3); d_list.reserve((size_t)total);
      g.start = d_start.p; g.ofirst = d_ofirst.p; g.nghost = (int)total;
      g.owner = d_owner.p; g.img = d_img.p; g.list = d_list.p;
      launch_ghost_images(ctx.stream, g, true);
      HIP_TRY(hipGetLastError());
      ctx.sync();
    }
  }
  nlocal = nl; nghost = (int)total;
  for (int c = 0; c < 3; ++c) prd[c] = g.prd[c];
  built = true;
  *nghost_out = nghost;
}

void GhostMap::fill(double *dx, double *dq) {
  need_built("conp_ghost_fill_device");
  if (!dx && nlocal + nghost > 0) throw ConpError(CONP_ERR_ARG, "conp_ghost_fill_device: d_x is NULL");
  if (nghost <= 0) return;
  launch_ghost_fill_xq(ctx.stream, nlocal, nghost, d_owner.p, d_img.p, prd[0], prd[1], prd[2], dx, dq);
  HIP_TRY(hipGetLastError());
}

void GhostMap::fill_int(int *dv, int width) {
  need_built("conp_ghost_fill_int_device");
  if (width < 1 || width > 8) throw ConpError(CONP_ERR_ARG, "conp_ghost_fill_int_device: width outside 1 .. 8");
  if (!dv && nlocal + nghost > 0) throw ConpError(CONP_ERR_ARG, "conp_ghost_fill_int_device: d_v is NULL");
  if (nghost <= 0) return;
  launch_ghost_fill_int(ctx.stream, nlocal, nghost, width, d_owner.p, dv);
  HIP_TRY(hipGetLastError());
}

void GhostMap::fold(double *dv, int width) {
  need_built("conp_ghost_fold_device");
  if (width != 1 && width != 3 && width != 6) throw ConpError(CONP_ERR_ARG, "conp_ghost_fold_device: width is not 1, 3 or 6");
  if (!dv && nlocal + nghost > 0) throw ConpError(CONP_ERR_ARG, "conp_ghost_fold_device: d_v is NULL");
  if (nghost <= 0) return;
  launch_ghost_fold(ctx.stream, nlocal, width, d_ofirst.p, d_nimg.p, d_list.p, dv);
  HIP_TRY(hipGetLastError());
}

void GhostMap::get(int *nlocal_out, int *nghost_out, int *owner, int *img) {
  need_built("conp_ghost_get");
  if (nlocal_out) *nlocal_out = nlocal;
  if (nghost_out) *nghost_out = nghost;
  if (owner && nghost > 0) HIP_TRY(hipMemcpyAsync(owner, d_owner.p, (size_t)nghost * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
  if (img && nghost > 0) HIP_TRY(hipMemcpyAsync(img, d_img.p, (size_t)nghost * 3 * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
  ctx.sync();
}

void atoms_wrap(DevCtx &ctx, double *dx, int nlocal_, const double *boxlo, const double *boxhi, const int *periodic, int *dimage) {
  if (!boxlo || !boxhi || !periodic) throw ConpError(CONP_ERR_ARG, "null argument");
  if (nlocal_ < 0) throw ConpError(CONP_ERR_ARG, "conp_atoms_wrap_device: negative nlocal");
  if (!dx && nlocal_ > 0) throw ConpError(CONP_ERR_ARG, "conp_atoms_wrap_device: d_x is NULL");
  AtomsWrapArgs w;
  w.nlocal = nlocal_;
  for (int c = 0; c < 3; ++c) {
    w.periodic[c] = periodic[c] != 0;
    if (w.periodic[c] && !(boxhi[c] > boxlo[c])) throw ConpError(CONP_ERR_ARG, "conp_atoms_wrap_device: boxhi <= boxlo in a periodic dimension");
    w.lo[c] = boxlo[c]; w.hi[c] = boxhi[c]; w.prd[c] = boxhi[c] - boxlo[c];
  }
  launch_atoms_wrap(ctx.stream, w, dx, dimage);
  HIP_TRY(hipGetLastError());
}

}  // namespace conp
