// Bonded forces of `bond_style harmonic` and `angle_style harmonic` -- conp_bonded_compute / conp_bonded_compute_device of
// include/conp_hip.h, DESIGN.md section 21.
//
// The arithmetic is LAMMPS' bond_harmonic.cpp / angle_harmonic.cpp @ 27May2021 with Bond::ev_tally / Angle::ev_tally, restated in the
// header.  Products are kept as written (fp contract off).  No output meets an atomic:
//
//   bonded_term_kernel    <EV>: one thread per term, bonds first, then angles.  Writes the term's record (BONDED_TERM_W doubles: the
//                         force on the first member, on the third, the energy, the six virial products) into scratch.  EV: the
//                         term's weighted tallies (ebond, eangle, virial[6]) are reduced over the workgroup in a fixed tree and
//                         stored as one row per workgroup.
//   bonded_finish_kernel  adds the rows in a fixed order: the scheme of pair_finish_kernel, nothing cleared, one workgroup.
//   bonded_gather_kernel  one thread per atom: walks the atom's (term, role) slots in the order conp_bonded_set_lists stored them,
//                         sums the records' shares from 0.0 and adds the force to f once; eatom / vatom are written for every
//                         row (0.0 for an atom in no term), f is touched only for atoms with slots.
#include <hip/hip_runtime.h>

#include "conp_kernels.h"

namespace conp {

namespace {

__device__ __forceinline__ double bonded_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// x_b seen from x_a: the closest image along a dimension of length prd (0: as it is); the product first, then the sum
__device__ __forceinline__ double bonded_image(double xa, double xb, double prd) {
#pragma clang fp contract(off)
  if (!(prd > 0.0)) return xb;
  const double d = xa - xb, h = prd / 2;
  const int s = d > h ? 1 : (d < -h ? -1 : 0);
  const double shift = (double)s * prd;
  return xb + shift;
}

template <bool EV>
__global__ __launch_bounds__(BONDED_BLOCK) void bonded_term_kernel(BondedArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[BONDED_BLOCK / 64][8];
  const int nterm = a.nbond + a.nangle;
  const int t = blockIdx.x * BONDED_BLOCK + threadIdx.x;
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (t < nterm) {
    double *rec = a.term + (size_t)t * BONDED_TERM_W;
    if (t < a.nbond) {
      const int i1 = a.bond[3 * (size_t)t], i2 = a.bond[3 * (size_t)t + 1], ty = a.bond[3 * (size_t)t + 2];
      const double *x1 = a.x + 3 * (size_t)i1, *x2 = a.x + 3 * (size_t)i2;
      const double x1x = x1[0], x1y = x1[1], x1z = x1[2];
      const double delx = x1x - bonded_image(x1x, x2[0], a.prd[0]);
      const double dely = x1y - bonded_image(x1y, x2[1], a.prd[1]);
      const double delz = x1z - bonded_image(x1z, x2[2], a.prd[2]);
      const double rsq = delx * delx + dely * dely + delz * delz;
      const double r = sqrt(rsq);
      const double dr = r - a.bcoef[2 * ty + 1];
      const double rk = a.bcoef[2 * ty] * dr;
      const double fbond = r > 0.0 ? -2.0 * rk / r : 0.0;
      const double ebond = rk * dr;
      double v[6];
      v[0] = fbond * (delx * delx); v[1] = fbond * (dely * dely); v[2] = fbond * (delz * delz);
      v[3] = fbond * (delx * dely); v[4] = fbond * (delx * delz); v[5] = fbond * (dely * delz);
      rec[0] = delx * fbond; rec[1] = dely * fbond; rec[2] = delz * fbond;
      rec[3] = 0.0; rec[4] = 0.0; rec[5] = 0.0;
      rec[6] = ebond;
#pragma unroll
      for (int k = 0; k < 6; ++k) rec[7 + k] = v[k];
      if (EV) {
        if (a.newton) {
          s[0] = ebond;
#pragma unroll
          for (int k = 0; k < 6; ++k) s[2 + k] = v[k];
        } else {
          const bool o1 = i1 < a.nlocal, o2 = i2 < a.nlocal;
          const double eh = 0.5 * ebond;
          if (o1) s[0] += eh;
          if (o2) s[0] += eh;
#pragma unroll
          for (int k = 0; k < 6; ++k) {
            const double vh = 0.5 * v[k];
            if (o1) s[2 + k] += vh;
            if (o2) s[2 + k] += vh;
          }
        }
      }
    } else {
      const int *an = a.angle + 4 * (size_t)(t - a.nbond);
      const int i1 = an[0], i2 = an[1], i3 = an[2], ty = an[3];
      const double *x1 = a.x + 3 * (size_t)i1, *x2 = a.x + 3 * (size_t)i2, *x3 = a.x + 3 * (size_t)i3;
      const double cx = x2[0], cy = x2[1], cz = x2[2];
      const double delx1 = bonded_image(cx, x1[0], a.prd[0]) - cx;
      const double dely1 = bonded_image(cy, x1[1], a.prd[1]) - cy;
      const double delz1 = bonded_image(cz, x1[2], a.prd[2]) - cz;
      const double rsq1 = delx1 * delx1 + dely1 * dely1 + delz1 * delz1;
      const double r1 = sqrt(rsq1);
      const double delx2 = bonded_image(cx, x3[0], a.prd[0]) - cx;
      const double dely2 = bonded_image(cy, x3[1], a.prd[1]) - cy;
      const double delz2 = bonded_image(cz, x3[2], a.prd[2]) - cz;
      const double rsq2 = delx2 * delx2 + dely2 * dely2 + delz2 * delz2;
      const double r2 = sqrt(rsq2);
      double c = delx1 * delx2 + dely1 * dely2 + delz1 * delz2;
      c /= r1 * r2;
      if (c > 1.0) c = 1.0;
      if (c < -1.0) c = -1.0;
      double sn = sqrt(1.0 - c * c);
      if (sn < 0.001) sn = 0.001;
      sn = 1.0 / sn;
      const double dtheta = acos(c) - a.acoef[2 * ty + 1];
      const double tk = a.acoef[2 * ty] * dtheta;
      const double eangle = tk * dtheta;
      const double aa = -2.0 * tk * sn;
      const double a11 = aa * c / rsq1;
      const double a12 = -aa / (r1 * r2);
      const double a22 = aa * c / rsq2;
      const double f1x = a11 * delx1 + a12 * delx2, f1y = a11 * dely1 + a12 * dely2, f1z = a11 * delz1 + a12 * delz2;
      const double f3x = a22 * delx2 + a12 * delx1, f3y = a22 * dely2 + a12 * dely1, f3z = a22 * delz2 + a12 * delz1;
      double v[6];
      v[0] = delx1 * f1x + delx2 * f3x; v[1] = dely1 * f1y + dely2 * f3y; v[2] = delz1 * f1z + delz2 * f3z;
      v[3] = delx1 * f1y + delx2 * f3y; v[4] = delx1 * f1z + delx2 * f3z; v[5] = dely1 * f1z + dely2 * f3z;
      rec[0] = f1x; rec[1] = f1y; rec[2] = f1z;
      rec[3] = f3x; rec[4] = f3y; rec[5] = f3z;
      rec[6] = eangle;
#pragma unroll
      for (int k = 0; k < 6; ++k) rec[7 + k] = v[k];
      if (EV) {
        if (a.newton) {
          s[1] = eangle;
#pragma unroll
          for (int k = 0; k < 6; ++k) s[2 + k] = v[k];
        } else {
          const bool o1 = i1 < a.nlocal, o2 = i2 < a.nlocal, o3 = i3 < a.nlocal;
          const double et = (1.0 / 3.0) * eangle;
          if (o1) s[1] += et;
          if (o2) s[1] += et;
          if (o3) s[1] += et;
#pragma unroll
          for (int k = 0; k < 6; ++k) {
            const double vt = (1.0 / 3.0) * v[k];
            if (o1) s[2 + k] += vt;
            if (o2) s[2 + k] += vt;
            if (o3) s[2 + k] += vt;
          }
        }
      }
    }
  }
  if (!EV) return;
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = bonded_wave_sum(s[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) red[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    double tsum = 0.0;
    for (int w = 0; w < BONDED_BLOCK / 64; ++w) tsum += red[w][threadIdx.x];
    a.part[8 * (size_t)blockIdx.x + threadIdx.x] = tsum;
  }
}

// ev[k] = sum over the rows of part[row][k], k < 8: every thread adds its rows in ascending order, then one fixed tree
__global__ __launch_bounds__(BONDED_FINISH) void bonded_finish_kernel(int nrows, const double *__restrict__ part, double *__restrict__ ev) {
#pragma clang fp contract(off)
  __shared__ double red[BONDED_FINISH / 64][8];
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int r = threadIdx.x; r < nrows; r += BONDED_FINISH) {
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] += part[8 * (size_t)r + k];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = bonded_wave_sum(s[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) red[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    double t = 0.0;
    for (int w = 0; w < BONDED_FINISH / 64; ++w) t += red[w][threadIdx.x];
    ev[threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(BONDED_BLOCK) void bonded_gather_kernel(BondedArgs a) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * BONDED_BLOCK + threadIdx.x;
  if (i >= a.nall) return;
  const bool active = a.newton || i < a.nlocal;
  const int b = a.slot_ptr[i], e = active ? a.slot_ptr[i + 1] : b;
  double fx = 0.0, fy = 0.0, fz = 0.0, ei = 0.0;
  double vi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = b; k < e; ++k) {
    const int sl = a.slot[k], t = sl >> 2, role = sl & 3;
    const double *rec = a.term + (size_t)t * BONDED_TERM_W;
    double w;
    if (t < a.nbond) {
      w = 0.5;
      if (role == 0) { fx += rec[0]; fy += rec[1]; fz += rec[2]; }
      else { fx -= rec[0]; fy -= rec[1]; fz -= rec[2]; }
    } else {
      w = 1.0 / 3.0;
      if (role == 0) { fx += rec[0]; fy += rec[1]; fz += rec[2]; }
      else if (role == 2) { fx += rec[3]; fy += rec[4]; fz += rec[5]; }
      else { fx -= rec[0] + rec[3]; fy -= rec[1] + rec[4]; fz -= rec[2] + rec[5]; }
    }
    if (a.eatom) ei += rec[6] * w;
    if (a.vatom) {
#pragma unroll
      for (int c = 0; c < 6; ++c) vi[c] += rec[7 + c] * w;
    }
  }
  if (a.f && e > b) { a.f[3 * (size_t)i] += fx; a.f[3 * (size_t)i + 1] += fy; a.f[3 * (size_t)i + 2] += fz; }
  if (a.eatom) a.eatom[i] = ei;
  if (a.vatom) {
#pragma unroll
    for (int c = 0; c < 6; ++c) a.vatom[6 * (size_t)i + c] = vi[c];
  }
}

}  // namespace

void launch_bonded(hipStream_t s, const BondedArgs &a, double *ev) {
  const int nterm = a.nbond + a.nangle, nrows = (nterm + BONDED_BLOCK - 1) / BONDED_BLOCK;
  if (nterm > 0) {
    if (ev) hipLaunchKernelGGL((bonded_term_kernel<true>), dim3(nrows), dim3(BONDED_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((bonded_term_kernel<false>), dim3(nrows), dim3(BONDED_BLOCK), 0, s, a);
  }
  if (ev) hipLaunchKernelGGL(bonded_finish_kernel, dim3(1), dim3(BONDED_FINISH), 0, s, nrows, a.part, ev);
  if ((a.f || a.eatom || a.vatom) && a.nall > 0)
    hipLaunchKernelGGL(bonded_gather_kernel, dim3((a.nall + BONDED_BLOCK - 1) / BONDED_BLOCK), dim3(BONDED_BLOCK), 0, s, a);
}

}  // namespace conp
