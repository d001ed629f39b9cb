// `compute potential/atom` on the device -- conp_potential_atom_device of include/conp_hip.h, DESIGN.md section 27.  Three kernels:
// the pair part gathered per selected atom by one wavefront in the order of section 26 (no float atomic), the gather of the targets'
// x and q into the exact-Ewald projection's padded block buffers, and the finish over the targets (k-space part, Gaussian self term,
// slab terms, volts).  All arithmetic is double, in the order written, no contraction.
#include "conp_kernels.h"

namespace conp {

namespace {
constexpr int POT_MASK = 0x3FFFFFFF;      // a list entry without its special bits (which this compute ignores)
constexpr double POT_PIS = 1.77245385090551602729;      // sqrt(pi)

// section 26's shuffle tree: v += lane[l + 32]; += [l + 16]; += 8; 4; 2; 1 -- lane 0 holds the sum
__device__ __forceinline__ double pot_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// potential_pair_kernel's pair body, operation for operation: dudq of a pair at rsq (the OWNER's orientation) whose types are
// (ti, tj) = (owner, neighbour) and of whose members ne2 carry the eta bit.  false: outside a cutoff, nothing is set.
__device__ __forceinline__ bool pot_pair_dudq(const PotPairArgs &a, double rsq, int ti, int tj, int ne2, double &dudq) {
#pragma clang fp contract(off)
  if (rsq < 1e-10) rsq = 1e-10;
  if (!(rsq < a.cutsq[ti * (a.ntypes + 1) + tj] && rsq < a.cut_coulsq)) return false;
  const double r = sqrt(rsq), grij = a.g_ewald * r;
  double expm2 = exp(-grij * grij), t = 1.0 / (1.0 + 0.3275911 * grij);
  double erfc_ = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429)))) * expm2;
  dudq = erfc_ / r;
  if (a.eta != 0.0 && ne2) {
    const double etarij = ne2 == 2 ? a.eta * r / sqrt(2.0) : a.eta * r;
    if (etarij < 5.8) {
      expm2 = exp(-etarij * etarij);
      t = 1.0 / (1.0 + 0.3275911 * etarij);
      erfc_ = t * (0.254829592 + t * (-0.284496736 + t * (1.421413741 + t * (-1.453152027 + t * 1.061405429)))) * expm2;
      dudq -= erfc_ / r;
    }
  }
  return true;
}

// One wavefront per row `at` of [0, ntotal), four per workgroup.  An unselected row is written 0.0 and does no pair work.  A selected
// row's lanes stride first over at's own row (if own_row[at] >= 0): term q_j dudq; then over at's transposed entries: the pairs in
// which it is the j, rsq in the OWNER's orientation, term q_owner dudq.  A partner without charge adds nothing (the reference's
// (qtmp || q[j]) gate; 0 dudq is 0 behind the rsq floor): its charge is tested before its coordinates are loaded.  The lane sums go
// through the shuffle tree and lane 0 stores once: the sum times scale_owned on an owned row, times scale_ghost on a ghost row.
__global__ __launch_bounds__(256) void pot_pair_kernel(PotPairArgs a, TransposedView tv) {
#pragma clang fp contract(off)
  const int at = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (at >= a.ntotal) return;
  const int fa = a.flags[at];
  if (!(fa & 1)) {
    if (lane == 0) a.pot[at] = 0.0;
    return;
  }
  const double xa = a.x[3 * (size_t)at], ya = a.x[3 * (size_t)at + 1], za = a.x[3 * (size_t)at + 2];
  const int ta = a.type[at], ea = (fa >> 1) & 1;
  double mine = 0.0;
  if (tv.own_row[at] >= 0) {                     // the pairs in which `at` is the owner
    const int *jl = a.neigh + a.first[at];
    const int jn = a.numneigh[at];
    for (int jj = lane; jj < jn; jj += 64) {
      const int j = jl[jj] & POT_MASK;
      const double qj = a.q[j];
      if (qj == 0.0) continue;
      const double delx = xa - a.x[3 * (size_t)j], dely = ya - a.x[3 * (size_t)j + 1], delz = za - a.x[3 * (size_t)j + 2];
      const double rsq = delx * delx + dely * dely + delz * delz;
      double dudq;
      if (!pot_pair_dudq(a, rsq, ta, a.type[j], ea + ((a.flags[j] >> 1) & 1), dudq)) continue;
      mine += qj * dudq;
    }
  }
  const int lo = tv.tr_ptr[at], hi = tv.tr_ptr[at + 1];
  for (int k = lo + lane; k < hi; k += 64) {     // the pairs in which `at` is the j, ascending slot order
    const int i = tv.tr_entry[k] & POT_MASK;
    const double qi = a.q[i];
    if (qi == 0.0) continue;
    const double delx = a.x[3 * (size_t)i] - xa, dely = a.x[3 * (size_t)i + 1] - ya, delz = a.x[3 * (size_t)i + 2] - za;
    const double rsq = delx * delx + dely * dely + delz * delz;
    double dudq;
    if (!pot_pair_dudq(a, rsq, a.type[i], ta, ((a.flags[i] >> 1) & 1) + ea, dudq)) continue;
    mine += qi * dudq;
  }
  mine = pot_wave_sum(mine);
  if (lane == 0) a.pot[at] = mine * (at < a.nlocal ? a.scale_owned : a.scale_ghost);
}

// xg [ntot][3], qg [ntot]: x and q of the nt targets, then padding atoms at the origin without charge up to whole blocks
__global__ __launch_bounds__(256) void pot_gather_kernel(int nt, int ntot, const int *__restrict__ targets, const double *__restrict__ x,
                                                         const double *__restrict__ q, double *__restrict__ xg, double *__restrict__ qg) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= ntot) return;
  double v[3] = {0.0, 0.0, 0.0}, c = 0.0;
  if (k < nt) {
    const int i = targets[k];
    v[0] = x[3 * (size_t)i]; v[1] = x[3 * (size_t)i + 1]; v[2] = x[3 * (size_t)i + 2];
    c = q[i];
  }
  xg[3 * (size_t)k] = v[0]; xg[3 * (size_t)k + 1] = v[1]; xg[3 * (size_t)k + 2] = v[2];
  qg[k] = c;
}

// the k-space tail of the host entry (potential_atom_tail) on the targets, then volts: one thread per target
__global__ __launch_bounds__(256) void pot_finish_kernel(PotFinishArgs a) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= a.nt) return;
  const int i = a.targets[k];
  double p = a.pot[i];
  p -= a.u[i];
  if (a.eta != 0.0 && (a.flags[i] & 2)) p += a.eta * a.q[i] * sqrt(2.0) / POT_PIS;
  if (a.slab) {
    const double z = a.x[3 * (size_t)i + 2];
    const double slabcorr = 2 * a.pi2vol * a.four[2], qsum = a.four[0];      // M = sum q z, Q = sum q of the owned atoms
    p += z * slabcorr;
    if (a.qsum) p -= a.pi2vol * qsum * z * z;
  }
  a.pot[i] = p * a.evs;
}
}  // namespace

void launch_pot_pair(hipStream_t s, const PotPairArgs &a, const TransposedView &t) {
  if (a.ntotal > 0) hipLaunchKernelGGL(pot_pair_kernel, dim3((a.ntotal + 3) / 4), dim3(256), 0, s, a, t);
}

void launch_pot_gather(hipStream_t s, int nt, int ntot, const int *targets, const double *x, const double *q, double *xg, double *qg) {
  if (ntot > 0) hipLaunchKernelGGL(pot_gather_kernel, dim3((ntot + 255) / 256), dim3(256), 0, s, nt, ntot, targets, x, q, xg, qg);
}

void launch_pot_finish(hipStream_t s, const PotFinishArgs &a) {
  if (a.nt > 0) hipLaunchKernelGGL(pot_finish_kernel, dim3((a.nt + 255) / 256), dim3(256), 0, s, a);
}

}  // namespace conp
