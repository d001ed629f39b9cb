// The provider-independent steps of the k-space query entries (DESIGN.md sections 11-15): what the exact Ewald entries
// (conp_ewaldquery.cpp) and the PPPM entries (conp_pppmmesh.cpp) share.  Header-only; nothing down to kspace_out_args makes a HIP call.
#pragma once
#include <cmath>
#include <vector>

#include "conp_dev.hpp"
#include "conp_kernels.h"

namespace conp {

constexpr double MY_PI = 3.14159265358979323846, MY_PIS = 1.77245385090551602729;

// what these steps read of conp_env (copied when the handle is created: nothing of it changes afterwards)
struct KspaceEnv { double g_ewald, qqrd2e; int slabflag; double zprd, slab_volfactor; };

// A running sum that keeps its rounding errors (Neumaier).  The host entries add the atoms one by one: 66 000 sites that share four
// charge values lose 1e-8 of Q in a plain loop (the partial sum climbs to 1e4 and every addition rounds the same way), which the
// Q L^2 / 12 and Q z^2 slab terms carry into the energy and the per-atom potential; the device entries' tree sums do not.
struct CompSum {
  double s = 0.0, c = 0.0;
  void add(double v) {
    const double t = s + v;
    c += std::fabs(s) >= std::fabs(v) ? (s - t) + v : (v - t) + s;
    s = t;
  }
  double value() const { return s + c; }
};
// the owned atoms that carry charge into idx; Q, Q2, M, M2 of them (this rank's) into four
inline void charged_owned(const conp_atoms *at, std::vector<int> &idx, double four[4]) {
  CompSum acc[4];
  for (int i = 0; i < at->nlocal; ++i) {
    const double q = at->q[i], z = at->x[3 * (size_t)i + 2];
    if (q == 0) continue;
    idx.push_back(i);
    acc[0].add(q); acc[1].add(q * q); acc[2].add(q * z); acc[3].add(q * z * z);
  }
  for (int c = 0; c < 4; ++c) four[c] = acc[c].value();
}
// energy from the first of the seven k-space sums and the four sums: what kspace_finish_kernel evaluates for the device entries
inline double kspace_energy(const KspaceEnv &env, double s0, double Q, double Q2, double M, double M2, double V, double L) {
  const double g = env.g_ewald;
  double e = s0 - g * Q2 / MY_PIS - 0.5 * MY_PI * Q * Q / (g * g * V);
  if (env.slabflag) e += 2.0 * MY_PI * (M * M - Q * M2 - Q * Q * L * L / 12.0) / V;
  return env.qqrd2e * e;
}
inline KspaceFinish kspace_finish_args(const KspaceEnv &env, double V, double L) {
  const double g = env.g_ewald;
  KspaceFinish a{};
  a.qs = env.qqrd2e; a.g_pis = g / MY_PIS; a.qcoef = 0.5 * MY_PI / (g * g * V);
  a.slab = env.slabflag ? 1 : 0; a.slab_pref = 2.0 * MY_PI / V; a.L2_12 = L * L / 12.0;
  return a;
}
// The parameter block of the force-output kernels.  four == NULL (the device entries): Q, M, M2 stay zero and ecoef lacks its
// factor Q -- kspace_out_from_sums completes the block on the device.  The host entries hand in their four sums.
inline EwForceOut kspace_out_args(const KspaceEnv &env, double V, double L, const double *four) {
  const double g = env.g_ewald;
  EwForceOut o{};
  o.qs = env.qqrd2e; o.selfc = 2.0 * g / MY_PIS; o.ecoef = 0.5 * MY_PI / (g * g * V);
  o.slab = env.slabflag ? 1 : 0;
  o.fz_pref = -4.0 * MY_PI / V; o.e_pref = 2.0 * MY_PI / V; o.L2_12 = L * L / 12.0;
  if (four) {
    const double Q = four[0];
    o.Q = Q; o.M = four[2]; o.M2 = four[3]; o.ecoef = 0.5 * MY_PI * Q / (g * g * V);
  }
  return o;
}
// Q, Q2, M, M2 of the n atoms of the device arrays into d_kf_sums[0..3] (the owner's: an Ewald or a PPPM handle allocates one)
inline void kspace_four_sums(dev::DevCtx &ctx, dev::DevBuf<double> &d_kf_sums, int n, const double *dx, const double *dq) {
  d_kf_sums.reserve((size_t)4 * (kspace_four_sums_workgroups(n) + 1));
  launch_kspace_four_sums(ctx.stream, n, dx, dq, d_kf_sums.p + 4, d_kf_sums.p);
}
// The per-atom outputs of a host entry: d_f [nlocal][3] is ADDED to fout, d_e and d_v overwrite eatom and vatom, at the n atoms idx.
// A NULL device pointer: not formed, nothing copied; a NULL host pointer: not wanted.  Synchronises.
inline void download_scatter(dev::DevCtx &ctx, int nlocal, const std::vector<int> &idx, int n, const double *d_f, const double *d_e,
                             const double *d_v, double *fout, double *eatom, double *vatom) {
  std::vector<double> hf, he, hv;
  const auto download = [&](const double *d, size_t count, std::vector<double> &h) {
    if (!d) return;
    h.resize(count);
    HIP_TRY(hipMemcpyAsync(h.data(), d, count * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  };
  download(d_v, 6 * (size_t)nlocal, hv); download(d_f, 3 * (size_t)nlocal, hf); download(d_e, nlocal, he);
  HIP_TRY(hipGetLastError());
  ctx.sync();
  for (int k = 0; k < n; ++k) {
    const int i = idx[k];
    if (fout && d_f) for (int c = 0; c < 3; ++c) fout[3 * (size_t)i + c] += hf[3 * (size_t)i + c];
    if (eatom && d_e) eatom[i] = he[i];
    if (vatom && d_v) for (int c = 0; c < 6; ++c) vatom[6 * (size_t)i + c] = hv[6 * (size_t)i + c];
  }
}

}  // namespace conp
