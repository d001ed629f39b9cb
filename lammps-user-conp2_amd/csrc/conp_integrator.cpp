// Velocity Verlet and the Nose-Hoover chain on the device (conp_integrate.hip).  set_params checks and uploads
// the per-atom tables, zeroes the chains and sizes every buffer a step needs: the step entries then allocate nothing, copy nothing to
// the host and never wait.  The chains of all groups are rows of d_state, twice: `initial` reads one half in every workgroup and
// writes the other, the host only remembers which half is current.
#include "conp_integrator.hpp"

#include <cmath>

namespace conp {
using namespace dev;

namespace {
bool positive(double v) { return std::isfinite(v) && v > 0.0; }
}

void Integrator::set_params(const conp_integrate_params *p) {
  have_params = false; is_setup = false;            // a refused call leaves the handle without an integrator
  if (p->ngroups < 1 || p->ngroups > CONP_INTEGRATE_MAX_GROUPS) throw ConpError(CONP_ERR_ARG, "conp_integrate_set_params: ngroups out of range");
  if (p->nlocal < 0 || p->ntypes < 0) throw ConpError(CONP_ERR_ARG, "conp_integrate_set_params: negative count");
  if (!p->type || !p->group || !p->mass || !p->style || !p->dof || !p->t_period) throw ConpError(CONP_ERR_ARG, "conp_integrate_set_params: null array");
  if (!positive(p->dt) || !positive(p->ftm2v) || !positive(p->mvv2e) || !positive(p->boltz))
    throw ConpError(CONP_ERR_ARG, "conp_integrate_set_params: dt, ftm2v, mvv2e and boltz must be positive and finite");
  for (int t = 1; t <= p->ntypes; ++t)
    if (!positive(p->mass[t])) throw ConpError(CONP_ERR_ARG, "conp_integrate_set_params: a mass is not positive and finite");
  IntegrateArgs a{};
  bool nvt = false;
  for (int g = 0; g < p->ngroups; ++g) {
    if (p->style[g] != 0 && p->style[g] != 1) throw ConpError(CONP_ERR_ARG, "conp_integrate_set_params: style is neither 0 (nve) nor 1 (nvt)");
    if (!positive(p->dof[g])) throw ConpError(CONP_ERR_ARG, "conp_integrate_set_params: dof is not positive and finite");
    if (p->style[g] && !positive(p->t_period[g])) throw ConpError(CONP_ERR_ARG, "conp_integrate_set_params: t_period of an nvt group is not positive and finite");
    a.style[g] = p->style[g];
    a.dof[g] = p->dof[g];
    a.t_freq[g] = p->style[g] ? 1.0 / p->t_period[g] : 0.0;
    nvt = nvt || p->style[g];
  }
  // every index a kernel will use is checked here, once
  for (int i = 0; i < p->nlocal; ++i) {
    if (p->type[i] < 1 || p->type[i] > p->ntypes) throw ConpError(CONP_ERR_ARG, "conp_integrate_set_params: type outside [1, ntypes]");
    if (p->group[i] < -1 || p->group[i] >= p->ngroups) throw ConpError(CONP_ERR_ARG, "conp_integrate_set_params: group outside [-1, ngroups)");
  }
  a.nlocal = p->nlocal; a.ngroups = p->ngroups;
  a.dtv = p->dt; a.dtf = 0.5 * p->dt * p->ftm2v; a.dthalf = 0.5 * p->dt; a.dt4 = 0.25 * p->dt; a.dt8 = 0.125 * p->dt;
  a.mvv2e = p->mvv2e; a.boltz = p->boltz;
  const size_t n = (size_t)p->nlocal;
  ctx.sync();                                       // no kernel may be reading the old tables
  d_type.upload(p->type, n, ctx.stream);
  d_group.upload(p->group, n, ctx.stream);
  d_mass.upload(p->mass, (size_t)p->ntypes + 1, ctx.stream);
  d_state.reserve(2 * (size_t)INTEGRATE_G * INTEGRATE_STATE_W);
  d_state.zero(ctx.stream);
  d_part.reserve(std::max<size_t>((n + INTEGRATE_BLOCK - 1) / INTEGRATE_BLOCK, 1) * INTEGRATE_G);
  d_factor.reserve(INTEGRATE_G);
  d_raw.reserve((size_t)INTEGRATE_G * 8);
  raw_h.assign((size_t)INTEGRATE_G * INTEGRATE_STATE_W, 0.0);
  ctx.sync();                                       // the caller's arrays need not stay
  a.type = d_type.p; a.group = d_group.p; a.mass = d_mass.p; a.part = d_part.p; a.factor = d_factor.p;
  proto = a;
  nlocal = p->nlocal; ngroups = p->ngroups; any_nvt = nvt; cur = 0;
  have_params = true;
}

IntegrateArgs Integrator::args(const double *t_target, const char *who) const {
  IntegrateArgs a = proto;
  if (!t_target) throw ConpError(CONP_ERR_ARG, std::string(who) + ": null t_target");
  for (int g = 0; g < ngroups; ++g) {
    const double t = t_target[g];
    if (!std::isfinite(t) || t < 0.0 || (a.style[g] && t == 0.0))
      throw ConpError(CONP_ERR_ARG, std::string(who) + ": t_target is negative, not finite, or 0 for an nvt group");
    a.t_target[g] = t;
  }
  return a;
}

void Integrator::setup(const double *d_v, const double *t_target) {
  IntegrateArgs a = args(t_target, "conp_integrate_setup_device");
  a.v = const_cast<double *>(d_v);                  // (the sums kernel without UPDATE only loads)
  a.state_in = state(cur); a.state_out = state(cur);
  ctx.prof.begin("integrate", ctx.stream);
  launch_integrate_sums(ctx.stream, a, false, INTEGRATE_SETUP, false);
  ctx.prof.end(ctx.stream);
  HIP_TRY(hipGetLastError());
  is_setup = true;
}

void Integrator::initial(double *d_x, double *d_v, const double *d_f, const double *t_target) {
  IntegrateArgs a = args(t_target, "conp_integrate_initial_device");
  if (nlocal == 0) return;
  a.x = d_x; a.v = d_v; a.f = d_f;
  a.state_in = state(cur); a.state_out = state(cur ^ 1);
  ctx.prof.begin("integrate", ctx.stream);
  launch_integrate_initial(ctx.stream, a);
  ctx.prof.end(ctx.stream);
  HIP_TRY(hipGetLastError());
  cur ^= 1;
}

void Integrator::final_(double *d_v, const double *d_f, double *d_out) {
  if (nlocal == 0) {
    if (d_out) HIP_TRY(hipMemsetAsync(d_out, 0, 4 * (size_t)ngroups * sizeof(double), ctx.stream));
    return;
  }
  IntegrateArgs a = proto;
  a.v = d_v; a.f = d_f; a.out = d_out;
  a.state_in = state(cur); a.state_out = state(cur);
  ctx.prof.begin("integrate", ctx.stream);
  launch_integrate_sums(ctx.stream, a, true, INTEGRATE_FINAL, any_nvt);
  ctx.prof.end(ctx.stream);
  HIP_TRY(hipGetLastError());
}

void Integrator::temperature(const double *d_v, double *d_out) {
  if (nlocal == 0) {
    HIP_TRY(hipMemsetAsync(d_out, 0, 4 * (size_t)ngroups * sizeof(double), ctx.stream));
    return;
  }
  IntegrateArgs a = proto;
  a.v = const_cast<double *>(d_v); a.out = d_out;
  a.state_in = state(cur); a.state_out = state(cur);
  ctx.prof.begin("integrate", ctx.stream);
  launch_integrate_sums(ctx.stream, a, false, INTEGRATE_TEMPERATURE, false);
  ctx.prof.end(ctx.stream);
  HIP_TRY(hipGetLastError());
}

void Integrator::get_state(double *state8) {
  HIP_TRY(hipMemcpyAsync(raw_h.data(), state(cur), (size_t)INTEGRATE_G * INTEGRATE_STATE_W * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  ctx.sync();
  for (int g = 0; g < ngroups; ++g) {
    const double *row = raw_h.data() + (size_t)g * INTEGRATE_STATE_W;
    for (int k = 0; k < 6; ++k) state8[8 * (size_t)g + k] = row[k];
    state8[8 * (size_t)g + 6] = row[9];
    state8[8 * (size_t)g + 7] = row[10];
  }
}

void Integrator::set_state(const double *state8) {
  for (int g = 0; g < ngroups; ++g) {
    const double *row = state8 + 8 * (size_t)g;
    for (int k = 0; k < 7; ++k)
      if (!std::isfinite(row[k])) throw ConpError(CONP_ERR_ARG, "conp_integrate_set_state: a state entry is not finite");
    if (!std::isfinite(row[7]) || row[7] < 0.0 || (proto.style[g] && row[7] == 0.0))
      throw ConpError(CONP_ERR_ARG, "conp_integrate_set_state: t_target is negative, not finite, or 0 for an nvt group");
  }
  IntegrateArgs a = proto;
  ctx.sync();
  d_raw.upload(state8, 8 * (size_t)ngroups, ctx.stream);
  a.state_in = d_raw.p; a.state_out = state(cur);
  launch_integrate_seed(ctx.stream, a);
  HIP_TRY(hipGetLastError());
  ctx.sync();                                       // the caller's array need not stay
  is_setup = true;
}

}  // namespace conp
