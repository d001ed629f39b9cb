// SHAKE constraints on the device (conp_shake.hip).  set_params checks every index and type a kernel will use,
// uploads the tables and sizes the scratch rows: the step entries then allocate nothing, copy nothing to the host and never wait.
#include "conp_shakestyle.hpp"

#include <algorithm>
#include <cmath>

namespace conp {
using namespace dev;

namespace {
bool positive(double v) { return std::isfinite(v) && v > 0.0; }
}

void ShakeStyle::set_params(const conp_shake_params *p) {
  have_params = false;                              // a refused call leaves the handle without constraints
  const char *who = "conp_shake_set_params: ";
  if (p->nlocal < 0 || p->ntypes < 0 || p->nbondtypes < 0 || p->nangletypes < 0 || p->ncluster < 0)
    throw ConpError(CONP_ERR_ARG, std::string(who) + "negative count");
  if ((p->ntypes > 0 && !p->mass) || (p->nbondtypes > 0 && !p->bond_distance) || (p->nangletypes > 0 && !p->angle_distance) ||
      (p->nlocal > 0 && !p->type) || (p->ncluster > 0 && !p->cluster))
    throw ConpError(CONP_ERR_ARG, std::string(who) + "null array");
  if (!positive(p->dt) || !positive(p->ftm2v) || !positive(p->tolerance))
    throw ConpError(CONP_ERR_ARG, std::string(who) + "dt, ftm2v and tolerance must be positive and finite");
  if (p->max_iter < 1) throw ConpError(CONP_ERR_ARG, std::string(who) + "max_iter < 1");
  for (int c = 0; c < 3; ++c)
    if (!std::isfinite(p->prd[c]) || p->prd[c] < 0.0) throw ConpError(CONP_ERR_ARG, std::string(who) + "prd is negative or not finite");
  for (int t = 1; t <= p->ntypes; ++t)
    if (!positive(p->mass[t])) throw ConpError(CONP_ERR_ARG, std::string(who) + "a mass is not positive and finite");
  for (int t = 1; t <= p->nbondtypes; ++t)
    if (!positive(p->bond_distance[t])) throw ConpError(CONP_ERR_ARG, std::string(who) + "a bond distance is not positive and finite");
  for (int t = 1; t <= p->nangletypes; ++t)
    if (!positive(p->angle_distance[t])) throw ConpError(CONP_ERR_ARG, std::string(who) + "an angle distance is not positive and finite");
  for (int i = 0; i < p->nlocal; ++i)
    if (p->type[i] < 1 || p->type[i] > p->ntypes) throw ConpError(CONP_ERR_ARG, std::string(who) + "type outside [1, ntypes]");
  std::vector<int> member((size_t)p->nlocal, 0);
  for (int k = 0; k < p->ncluster; ++k) {
    const int *c = p->cluster + 7 * (size_t)k;
    const int flag = c[0];
    if (flag < 1 || flag > 3) throw ConpError(CONP_ERR_ARG, std::string(who) + "flag outside {1, 2, 3} (4, three bonds, is not supported)");
    const int natom = flag == 2 ? 2 : 3, nbond = flag == 2 ? 1 : 2;
    for (int m = 0; m < natom; ++m) {
      const int i = c[1 + m];
      if (i < 0 || i >= p->nlocal) throw ConpError(CONP_ERR_ARG, std::string(who) + "index outside [0, nlocal)");
      for (int l = 0; l < m; ++l)
        if (c[1 + l] == i) throw ConpError(CONP_ERR_ARG, std::string(who) + "an index is repeated in a cluster");
    }
    for (int m = 0; m < natom; ++m) {
      if (member[c[1 + m]]) throw ConpError(CONP_ERR_ARG, std::string(who) + "an atom is in two clusters");
      member[c[1 + m]] = 1;
    }
    for (int m = 0; m < nbond; ++m)
      if (c[4 + m] < 1 || c[4 + m] > p->nbondtypes) throw ConpError(CONP_ERR_ARG, std::string(who) + "bond type outside [1, nbondtypes]");
    if (flag == 1 && (c[6] < 1 || c[6] > p->nangletypes)) throw ConpError(CONP_ERR_ARG, std::string(who) + "angle type outside [1, nangletypes]");
  }
  ShakeArgs a{};
  a.ncluster = p->ncluster; a.nlocal = p->nlocal; a.max_iter = p->max_iter;
  a.dtv = p->dt; a.tolerance = p->tolerance;
  for (int c = 0; c < 3; ++c) a.prd[c] = p->prd[c];
  ctx.sync();                                       // no kernel may be reading the old tables
  d_type.upload(p->type, (size_t)p->nlocal, ctx.stream);
  d_member.upload(member, ctx.stream);
  d_cluster.upload(p->cluster, 7 * (size_t)p->ncluster, ctx.stream);
  // (a table without types may be NULL: no checked cluster or atom refers to it)
  d_mass.upload(p->mass, p->ntypes ? (size_t)p->ntypes + 1 : 0, ctx.stream);
  d_bond_d.upload(p->bond_distance, p->nbondtypes ? (size_t)p->nbondtypes + 1 : 0, ctx.stream);
  d_angle_d.upload(p->angle_distance, p->nangletypes ? (size_t)p->nangletypes + 1 : 0, ctx.stream);
  d_part.reserve((size_t)std::max(shake_rows(std::max(p->ncluster, p->nlocal)), 1) * SHAKE_PART_W);
  ctx.sync();                                       // the caller's arrays need not stay
  a.cluster = d_cluster.p; a.type = d_type.p; a.member = d_member.p;
  a.mass = d_mass.p; a.bond_d = d_bond_d.p; a.angle_d = d_angle_d.p;
  proto = a;
  nlocal = p->nlocal; ncluster = p->ncluster; dt = p->dt; ftm2v = p->ftm2v;
  have_params = true;
}

void ShakeStyle::correct(double *d_x) {
  if (ncluster == 0) return;
  ShakeArgs a = proto;
  a.dtfsq = 0.5 * dt * dt * ftm2v;
  a.x = d_x;
  ctx.prof.begin("shake", ctx.stream);
  launch_shake(ctx.stream, a, SHAKE_CORRECT, nullptr);
  ctx.prof.end(ctx.stream);
  HIP_TRY(hipGetLastError());
}

void ShakeStyle::force(const double *d_x, const double *d_v, double *d_f, double *d_out, double *d_vatom, bool setup) {
  if (ncluster == 0) {
    if (d_out) HIP_TRY(hipMemsetAsync(d_out, 0, SHAKE_PART_W * sizeof(double), ctx.stream));
    return;
  }
  ShakeArgs a = proto;
  a.dtfsq = setup ? 0.5 * dt * dt * ftm2v : dt * dt * ftm2v;
  a.x = const_cast<double *>(d_x);                  // (SHAKE_FORCE only loads x)
  a.v = d_v; a.f = d_f; a.vatom = d_vatom;
  a.part = d_out ? d_part.p : nullptr;
  ctx.prof.begin("shake", ctx.stream);
  launch_shake(ctx.stream, a, SHAKE_FORCE, d_out);
  ctx.prof.end(ctx.stream);
  HIP_TRY(hipGetLastError());
}

void ShakeStyle::check(const double *d_x, double *d_out) {
  if (ncluster == 0) {
    HIP_TRY(hipMemsetAsync(d_out, 0, 2 * sizeof(double), ctx.stream));
    return;
  }
  ShakeArgs a = proto;
  a.x = const_cast<double *>(d_x);
  a.part = d_part.p;
  ctx.prof.begin("shake", ctx.stream);
  launch_shake_check(ctx.stream, a, d_out);
  ctx.prof.end(ctx.stream);
  HIP_TRY(hipGetLastError());
}

}  // namespace conp
