// LAMMPS' `fix efield` with a constant field (optionally coupled to the fix scalar of the same update), and the per-group sums behind
// the decks' thermo columns -- the conp_efield_* and conp_observe_* entries of include/conp_hip.h, DESIGN.md section 24.
//
// All arithmetic is double in the order the header writes it, products left to right, fp contract off.  No sum meets an atomic:
//
//   efield_kernel          one thread per owned atom.  A selected atom adds q E to its row of f and, with d_vatom, stores its six virial
//                          terms; an unselected row of d_vatom is zeroed by the same launch.  With d_out the eleven terms go through a
//                          fixed tree over the workgroup into one row of partial sums per workgroup.  Coupled: every thread forms
//                          ez = qe2f (e2 + couple_scale s) from the handle's scalar slot (a uniform load), no launch of its own.
//   efield_finish_kernel   one workgroup: adds the rows in a fixed order (the scheme of integrate_finish_kernel) -> d_out [11].
//   observe_kernel         workgroup (b, g): one thread per owned atom of block b, for group g (blockIdx.y).  A member loads its atom
//                          once and keeps its ten terms in registers (the others hold zeros); a fixed 64-lane tree runs per column.
//                          Measured against a loop over the groups inside one workgroup per block, and against skipping the trees
//                          of a wave without a member: section 24.
//   observe_finish_kernel  one workgroup per group, the same scheme -> d_out [ngroups][10].
//
// Rows from nlocal on are neither loaded nor stored; unselected rows of f and atoms in no group are not loaded beyond sel / mask.  No
// thread returns before a barrier.
#include <hip/hip_runtime.h>

#include "conp_kernels.h"

namespace conp {

namespace {

__device__ __forceinline__ double field_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// u_c = x_c + ((double)image_c prd_c): the ghost arithmetic of section 18
__device__ __forceinline__ void unwrapped(const double *x, const int *image, const double (&prd)[3], size_t o, double (&u)[3]) {
#pragma clang fp contract(off)
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    u[c] = x[o + c];
    if (image) u[c] = u[c] + ((double)image[o + c] * prd[c]);
  }
}

__global__ __launch_bounds__(EFIELD_BLOCK) void efield_kernel(EfieldArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[EFIELD_BLOCK / 64][EFIELD_W];
  const int i = blockIdx.x * EFIELD_BLOCK + threadIdx.x;
  const double ez = a.scalar ? a.qe2f * (a.e2 + a.couple_scale * a.scalar[0]) : a.ez;
  double t[EFIELD_W];
#pragma unroll
  for (int k = 0; k < EFIELD_W; ++k) t[k] = 0.0;
  if (i < a.nlocal) {
    const size_t o = 3 * (size_t)i;
    if (a.sel[i] != 0) {
      const double q = a.q[i];
      double u[3];
      unwrapped(a.x, a.image, a.prd, o, u);
      const double fx = q * a.ex, fy = q * a.ey, fz = q * ez;
      a.f[o] += fx; a.f[o + 1] += fy; a.f[o + 2] += fz;
      t[0] = -((fx * u[0] + fy * u[1]) + fz * u[2]);
      t[1] = fx; t[2] = fy; t[3] = fz;
      t[4] = fx * u[0]; t[5] = fy * u[1]; t[6] = fz * u[2];
      t[7] = fx * u[1]; t[8] = fx * u[2]; t[9] = fy * u[2];
      t[10] = 1.0;
    }
    if (a.vatom) {
      double *row = a.vatom + 6 * (size_t)i;
#pragma unroll
      for (int k = 0; k < 6; ++k) row[k] = t[4 + k];
    }
  }
  if (a.part) {                                   // (uniform over the launch)
#pragma unroll
    for (int k = 0; k < EFIELD_W; ++k) t[k] = field_wave_sum(t[k]);
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
      for (int k = 0; k < EFIELD_W; ++k) red[threadIdx.x >> 6][k] = t[k];
    }
    __syncthreads();
    if (threadIdx.x < EFIELD_W) {
      double s = 0.0;
      for (int w = 0; w < EFIELD_BLOCK / 64; ++w) s += red[w][threadIdx.x];
      a.part[EFIELD_W * (size_t)blockIdx.x + threadIdx.x] = s;
    }
  }
}

__global__ __launch_bounds__(EFIELD_FINISH) void efield_finish_kernel(const double *part, int nrows, double *out) {
#pragma clang fp contract(off)
  __shared__ double red[EFIELD_FINISH / 64][EFIELD_W];
  double s[EFIELD_W];
#pragma unroll
  for (int k = 0; k < EFIELD_W; ++k) s[k] = 0.0;
  for (int r = threadIdx.x; r < nrows; r += EFIELD_FINISH) {
#pragma unroll
    for (int k = 0; k < EFIELD_W; ++k) s[k] += part[EFIELD_W * (size_t)r + k];
  }
#pragma unroll
  for (int k = 0; k < EFIELD_W; ++k) s[k] = field_wave_sum(s[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < EFIELD_W; ++k) red[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < EFIELD_W) {
    double t = 0.0;
    for (int w = 0; w < EFIELD_FINISH / 64; ++w) t += red[w][threadIdx.x];
    out[threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(OBSERVE_BLOCK) void observe_kernel(ObserveArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[OBSERVE_BLOCK / 64][OBSERVE_W];
  const int g = blockIdx.y;
  const int i = blockIdx.x * OBSERVE_BLOCK + threadIdx.x;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  bool in = false;
  double c[OBSERVE_W];
#pragma unroll
  for (int k = 0; k < OBSERVE_W; ++k) c[k] = 0.0;
  if (i < a.nlocal) in = (((unsigned)a.mask[i]) >> g) & 1u;
  if (in) {
    const size_t o = 3 * (size_t)i;
    const double q = a.q[i], m = a.mass[a.type[i]];
    double u[3];
    unwrapped(a.x, a.image, a.prd, o, u);
    c[0] = 1.0; c[1] = q;
    c[2] = q * u[0]; c[3] = q * u[1]; c[4] = q * u[2];
    if (a.v) {
      const double vx = a.v[o], vy = a.v[o + 1], vz = a.v[o + 2];
      c[5] = m * ((vx * vx + vy * vy) + vz * vz);
      c[6] = m * vx; c[7] = m * vy; c[8] = m * vz;
    }
    c[9] = m;
  }
#pragma unroll
  for (int k = 0; k < OBSERVE_W; ++k) {
    double s = 0.0;
    if (a.v || k < 5 || k > 8) s = field_wave_sum(c[k]);
    if (lane == 0) red[wave][k] = s;
  }
  __syncthreads();
  if (threadIdx.x < OBSERVE_W) {
    double s = 0.0;
    for (int w = 0; w < OBSERVE_BLOCK / 64; ++w) s += red[w][threadIdx.x];
    a.part[((size_t)blockIdx.x * a.ngroups + g) * OBSERVE_W + threadIdx.x] = s;
  }
}

// workgroup g finishes group g
__global__ __launch_bounds__(OBSERVE_FINISH) void observe_finish_kernel(const double *part, int nrows, int ngroups, double *out) {
#pragma clang fp contract(off)
  __shared__ double red[OBSERVE_FINISH / 64][OBSERVE_W];
  const int g = blockIdx.x;
  const size_t ncol = (size_t)ngroups * OBSERVE_W;
  double s[OBSERVE_W];
#pragma unroll
  for (int k = 0; k < OBSERVE_W; ++k) s[k] = 0.0;
  for (int r = threadIdx.x; r < nrows; r += OBSERVE_FINISH) {
    const double *row = part + (size_t)r * ncol + (size_t)g * OBSERVE_W;
#pragma unroll
    for (int k = 0; k < OBSERVE_W; ++k) s[k] += row[k];
  }
#pragma unroll
  for (int k = 0; k < OBSERVE_W; ++k) s[k] = field_wave_sum(s[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < OBSERVE_W; ++k) red[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < OBSERVE_W) {
    double t = 0.0;
    for (int w = 0; w < OBSERVE_FINISH / 64; ++w) t += red[w][threadIdx.x];
    out[(size_t)g * OBSERVE_W + threadIdx.x] = t;
  }
}

}  // namespace

void launch_efield(hipStream_t s, const EfieldArgs &a, double *out) {
  const int nrows = efield_rows(a.nlocal);
  if (nrows > 0) hipLaunchKernelGGL(efield_kernel, dim3(nrows), dim3(EFIELD_BLOCK), 0, s, a);
  if (out) hipLaunchKernelGGL(efield_finish_kernel, dim3(1), dim3(EFIELD_FINISH), 0, s, a.part, nrows, out);
}

void launch_observe(hipStream_t s, const ObserveArgs &a, double *out) {
  const int nrows = observe_rows(a.nlocal);
  if (nrows > 0) hipLaunchKernelGGL(observe_kernel, dim3(nrows, a.ngroups), dim3(OBSERVE_BLOCK), 0, s, a);
  hipLaunchKernelGGL(observe_finish_kernel, dim3(a.ngroups), dim3(OBSERVE_FINISH), 0, s, a.part, nrows, a.ngroups, out);
}

}  // namespace conp
