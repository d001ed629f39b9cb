// `fix efield` and the per-group thermo sums on the device (conp_efield.hip).  set_params checks every index a
// kernel will use, uploads the tables and sizes the scratch rows: the step entries then allocate nothing, copy nothing to the host
// and never wait.
#include "conp_fieldstyle.hpp"

#include <algorithm>
#include <cmath>
#include <vector>

namespace conp {
using namespace dev;

namespace {
bool positive(double v) { return std::isfinite(v) && v > 0.0; }
void check_prd(const double *prd, const std::string &who) {
  for (int c = 0; c < 3; ++c)
    if (!std::isfinite(prd[c]) || prd[c] < 0.0) throw ConpError(CONP_ERR_ARG, who + "prd is negative or not finite");
}
}

void FieldStyle::set_params(const conp_efield_params *p) {
  have_params = false;                              // a refused call leaves the handle without a field
  const std::string who = "conp_efield_set_params: ";
  if (p->nlocal < 0) throw ConpError(CONP_ERR_ARG, who + "negative nlocal");
  if (p->nlocal > 0 && !p->sel) throw ConpError(CONP_ERR_ARG, who + "null sel");
  if (!std::isfinite(p->qe2f)) throw ConpError(CONP_ERR_ARG, who + "qe2f is not finite");
  check_prd(p->prd, who);
  std::vector<int> sel((size_t)p->nlocal);
  for (int i = 0; i < p->nlocal; ++i) sel[i] = p->sel[i] != 0;
  EfieldArgs a{};
  a.nlocal = p->nlocal; a.qe2f = p->qe2f;
  for (int c = 0; c < 3; ++c) a.prd[c] = p->prd[c];
  ctx.sync();                                       // no kernel may be reading the old table
  d_sel.upload(sel, ctx.stream);
  d_part.reserve((size_t)std::max(efield_rows(p->nlocal), 1) * EFIELD_W);
  ctx.sync();                                       // the caller's array need not stay
  a.sel = d_sel.p;
  proto = a;
  nlocal = p->nlocal;
  have_params = true;
}

void FieldStyle::post_force(const double *d_x, const double *d_q, const int *d_image, double *d_f, const double *e, const double *d_scalar,
                            double couple_scale, double *d_out, double *d_vatom) {
  if (nlocal == 0) {
    if (d_out) HIP_TRY(hipMemsetAsync(d_out, 0, EFIELD_W * sizeof(double), ctx.stream));
    return;
  }
  EfieldArgs a = proto;
  a.x = d_x; a.q = d_q; a.image = d_image; a.f = d_f;
  a.ex = a.qe2f * e[0]; a.ey = a.qe2f * e[1]; a.ez = a.qe2f * e[2];
  a.e2 = e[2]; a.couple_scale = couple_scale; a.scalar = d_scalar;
  a.vatom = d_vatom;
  a.part = d_out ? d_part.p : nullptr;
  ctx.prof.begin("efield", ctx.stream);
  launch_efield(ctx.stream, a, d_out);
  ctx.prof.end(ctx.stream);
  HIP_TRY(hipGetLastError());
}

void ObserveStyle::set_params(const conp_observe_params *p) {
  have_params = false;                              // a refused call leaves the handle without groups
  const std::string who = "conp_observe_set_params: ";
  if (p->ngroups < 1 || p->ngroups > CONP_OBSERVE_MAX_GROUPS) throw ConpError(CONP_ERR_ARG, who + "ngroups out of range");
  if (p->nlocal < 0 || p->ntypes < 0) throw ConpError(CONP_ERR_ARG, who + "negative count");
  if ((p->nlocal > 0 && (!p->type || !p->mask)) || (p->ntypes > 0 && !p->mass)) throw ConpError(CONP_ERR_ARG, who + "null array");
  check_prd(p->prd, who);
  for (int t = 1; t <= p->ntypes; ++t)
    if (!positive(p->mass[t])) throw ConpError(CONP_ERR_ARG, who + "a mass is not positive and finite");
  // every index a kernel will use is checked here, once
  const unsigned allowed = p->ngroups >= 32 ? ~0u : (1u << p->ngroups) - 1u;
  for (int i = 0; i < p->nlocal; ++i) {
    if (p->type[i] < 1 || p->type[i] > p->ntypes) throw ConpError(CONP_ERR_ARG, who + "type outside [1, ntypes]");
    if ((unsigned)p->mask[i] & ~allowed) throw ConpError(CONP_ERR_ARG, who + "a mask bit at or above ngroups");
  }
  ObserveArgs a{};
  a.nlocal = p->nlocal; a.ngroups = p->ngroups;
  for (int c = 0; c < 3; ++c) a.prd[c] = p->prd[c];
  ctx.sync();                                       // no kernel may be reading the old tables
  d_type.upload(p->type, (size_t)p->nlocal, ctx.stream);
  d_mask.upload(p->mask, (size_t)p->nlocal, ctx.stream);
  d_mass.upload(p->mass, p->ntypes ? (size_t)p->ntypes + 1 : 0, ctx.stream);
  d_part.reserve((size_t)std::max(observe_rows(p->nlocal), 1) * p->ngroups * OBSERVE_W);
  ctx.sync();                                       // the caller's arrays need not stay
  a.type = d_type.p; a.mask = d_mask.p; a.mass = d_mass.p; a.part = d_part.p;
  proto = a;
  nlocal = p->nlocal; ngroups = p->ngroups;
  have_params = true;
}

void ObserveStyle::observe(const double *d_x, const double *d_q, const double *d_v, const int *d_image, double *d_out) {
  if (nlocal == 0) {
    HIP_TRY(hipMemsetAsync(d_out, 0, (size_t)ngroups * OBSERVE_W * sizeof(double), ctx.stream));
    return;
  }
  ObserveArgs a = proto;
  a.x = d_x; a.q = d_q; a.v = d_v; a.image = d_image;
  ctx.prof.begin("observe", ctx.stream);
  launch_observe(ctx.stream, a, d_out);
  ctx.prof.end(ctx.stream);
  HIP_TRY(hipGetLastError());
}

}  // namespace conp
