// `fix zmirror` on the device (conp_zmirror.hip).  set_params restates FixZmirror::setup and the one-rank
// branch of FixZmirror::post_integrate once: the tag ranges of the two groups, then for every owned atom of the sending group the
// owned atom whose tag has the same offset in the receiving range.  Every index the kernel will use is checked here; the step entry
// then launches one kernel and nothing else.
#include "conp_zmirrorstyle.hpp"

#include <algorithm>
#include <cmath>
#include <unordered_map>

namespace conp {
using namespace dev;

void ZmirrorStyle::set_params(const conp_zmirror_params *p) {
  have_params = false;                              // a refused call leaves the handle without a mirror
  const std::string who = "conp_zmirror_set_params: ";
  if (p->nlocal < 0) throw ConpError(CONP_ERR_ARG, who + "negative nlocal");
  if (!p->tag || !p->mask) throw ConpError(CONP_ERR_ARG, who + "null tag or mask");
  if (p->nevery < 1) throw ConpError(CONP_ERR_ARG, who + "nevery below 1");
  if (!std::isfinite(p->boxlo_z) || !std::isfinite(p->zprd)) throw ConpError(CONP_ERR_ARG, who + "boxlo_z or zprd is not finite");
  std::unordered_map<int, int> at;                  // tag -> owned index
  at.reserve((size_t)p->nlocal * 2);
  bool send = false, recv = false;
  long long smin = 0, smax = 0, rmin = 0, rmax = 0;
  for (int i = 0; i < p->nlocal; ++i) {
    if (!at.emplace(p->tag[i], i).second) throw ConpError(CONP_ERR_ARG, who + "a tag occurs twice");
    const long long t = p->tag[i];
    if (p->mask[i] & p->groupbit) { smin = send ? std::min(smin, t) : t; smax = send ? std::max(smax, t) : t; send = true; }
    if (p->mask[i] & p->jgroupbit) { rmin = recv ? std::min(rmin, t) : t; rmax = recv ? std::max(rmax, t) : t; recv = true; }
  }
  if (!send) throw ConpError(CONP_ERR_ARG, who + "the sending group is empty");
  if (!recv) throw ConpError(CONP_ERR_ARG, who + "the receiving group is empty");
  if (smax - smin != rmax - rmin) throw ConpError(CONP_ERR_ARG, who + "Groups do not have same number of tags");
  std::vector<int> src, dst;
  std::vector<int2> map;
  for (int i = 0; i < p->nlocal; ++i) {
    if (!(p->mask[i] & p->groupbit)) continue;
    const long long want = (long long)p->tag[i] - smin + rmin;
    const auto it = want >= INT32_MIN && want <= INT32_MAX ? at.find((int)want) : at.end();
    if (it == at.end()) throw ConpError(CONP_ERR_ARG, who + "no owned atom has the tag a sending atom maps to");
    const int j = it->second;
    if (!(p->mask[j] & p->jgroupbit)) throw ConpError(CONP_ERR_ARG, who + "a target is outside the receiving group");
    if (p->mask[j] & p->groupbit) throw ConpError(CONP_ERR_ARG, who + "a target is itself in the sending group");
    src.push_back(i); dst.push_back(j);
    map.push_back(make_int2(i, j));
  }
  ctx.sync();                                       // no kernel may be reading the old map
  d_map.upload(map, ctx.stream);
  ctx.sync();                                       // `map` leaves scope
  src_h.swap(src); dst_h.swap(dst);
  npairs = (int)src_h.size();
  nevery = p->nevery;
  zoffset = 2 * p->boxlo_z + p->zprd;               // as FixZmirror::post_integrate forms it
  have_params = true;
}

void ZmirrorStyle::post_integrate(double *d_x, long long ntimestep) {
  if (ntimestep % nevery != 0) return;
  ctx.prof.begin("zmirror", ctx.stream);
  launch_zmirror(ctx.stream, npairs, d_map.p, zoffset, d_x);
  ctx.prof.end(ctx.stream);
  HIP_TRY(hipGetLastError());
}

}  // namespace conp
