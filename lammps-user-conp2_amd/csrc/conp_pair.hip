// Real-space pair forces of `pair_style lj/cut/coul/long` (and coul/long: no LJ tables) over a flattened LAMMPS half list --
// conp_pair_compute / conp_pair_compute_device of include/conp_hip.h, DESIGN.md section 16.
//
// The arithmetic is LAMMPS' pair_lj_cut_coul_long.cpp @ 27May2021 with ncoultablebits = 0, restated in the header: the 5-term erfc
// polynomial is part of the definition, as it is for the A matrix.  Products are kept as written (fp contract off).
//
//   pair_pack_kernel     x[nall][3], q[nall] -> one 32-byte record per atom, so that a neighbour costs one gather
//   pair_force_kernel    <EV, ATOM, LDS>: one wavefront per list owner, four per workgroup; lanes stride over the owner's neighbours.
//                        The owner's force (and its eatom / vatom share) is accumulated in registers, reduced across the wave and
//                        added once; the j side is added per pair.  Both with atomics: an atom is owner of one row and j of others.
//                        EV: the eight sums (eng_vdwl, eng_coul, virial[6]) are reduced per wave and written as one row per owner.
//                        LDS: the per-type-pair table sits in LDS (up to PAIR_LDS_ENTRIES type pairs); else it is read from global.
//   pair_finish_kernel   adds the rows in a fixed order (no atomics): energy and virial are bit-reproducible from run to run.
#include <hip/hip_runtime.h>

#include "conp_kernels.h"

namespace conp {

namespace {

constexpr int PAIR_MASK = 0x3FFFFFFF;

__device__ __forceinline__ double pair_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__global__ __launch_bounds__(256) void pair_pack_kernel(int nall, const double *__restrict__ x, const double *__restrict__ q,
                                                        double4 *__restrict__ xq) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nall) return;
  xq[i] = make_double4(x[3 * (size_t)i], x[3 * (size_t)i + 1], x[3 * (size_t)i + 2], q[i]);
}

template <bool EV, bool ATOM, bool LDS>
__global__ __launch_bounds__(256) void pair_force_kernel(PairArgs a) {
#pragma clang fp contract(off)
  __shared__ double tab_s[LDS ? PAIR_LDS_ENTRIES * PAIR_TAB_W : 1];
  const double *tab = a.tab;
  if (LDS) {
    for (int k = threadIdx.x; k < a.ntab * PAIR_TAB_W; k += 256) tab_s[k] = a.tab[k];
    __syncthreads();
    tab = tab_s;
  }
  const int ii = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (ii >= a.inum) return;                      // (whole waves leave, after the only barrier)
  const int i = a.ilist[ii];
  const int *jl = a.neigh + a.first[i];
  const int jn = a.numneigh[i];
  const double4 pi = a.xq[i];
  const int trow = a.type[i] * a.nt1;
  const bool iw = a.newton || i < a.nlocal;      // i receives its force / per-atom share (a list owner is owned: always)
  double fx = 0.0, fy = 0.0, fz = 0.0, ei = 0.0;
  double vi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int jj = lane; jj < jn; jj += 64) {
    const int jraw = jl[jj];
    const int sb = (jraw >> 30) & 3, j = jraw & PAIR_MASK;
    const double4 pj = a.xq[j];
    const double delx = pi.x - pj.x, dely = pi.y - pj.y, delz = pi.z - pj.z;
    const double rsq = delx * delx + dely * dely + delz * delz;
    const double *t = tab + (size_t)(trow + a.type[j]) * PAIR_TAB_W;      // cutsq, cut_ljsq, lj1, lj2, lj3, lj4, offset
    if (!(rsq < t[0])) continue;
    const double fc = a.special_coul[sb], fl = a.special_lj[sb];
    const double r2inv = 1.0 / rsq;
    double forcecoul = 0.0, ecoul = 0.0, forcelj = 0.0, evdwl = 0.0;
    if (rsq < a.cut_coulsq) {
      const double r = sqrt(rsq);
      const double grij = a.g_ewald * r;
      const double expm2 = exp(-grij * grij);
      const double tt = 1.0 / (1.0 + 0.3275911 * grij);
      const double erfc_ = tt * (0.254829592 + tt * (-0.284496736 + tt * (1.421413741 + tt * (-1.453152027 + tt * 1.061405429)))) * expm2;
      const double prefactor = a.qqrd2e * pi.w * pj.w / r;
      forcecoul = prefactor * (erfc_ + 1.12837917 * grij * expm2);
      if (fc < 1.0) forcecoul -= (1.0 - fc) * prefactor;
      if (EV || ATOM) {
        ecoul = prefactor * erfc_;
        if (fc < 1.0) ecoul -= (1.0 - fc) * prefactor;
      }
    }
    if (rsq < t[1]) {
      const double r6inv = r2inv * r2inv * r2inv;
      forcelj = r6inv * (t[2] * r6inv - t[3]);
      if (EV || ATOM) evdwl = fl * (r6inv * (t[4] * r6inv - t[5]) - t[6]);
    }
    const double fpair = (forcecoul + fl * forcelj) * r2inv;
    const bool jw = a.newton || j < a.nlocal;
    fx += delx * fpair; fy += dely * fpair; fz += delz * fpair;
    if (a.f && jw) {
      atomicAdd(&a.f[3 * (size_t)j], -(delx * fpair));
      atomicAdd(&a.f[3 * (size_t)j + 1], -(dely * fpair));
      atomicAdd(&a.f[3 * (size_t)j + 2], -(delz * fpair));
    }
    if (EV || ATOM) {
      const double v[6] = {delx * delx * fpair, dely * dely * fpair, delz * delz * fpair,
                           delx * dely * fpair, delx * delz * fpair, dely * delz * fpair};
      if (EV) {
        double w = 1.0;
        if (!a.newton) w = (i < a.nlocal ? 0.5 : 0.0) + (j < a.nlocal ? 0.5 : 0.0);
        s[0] += w * evdwl; s[1] += w * ecoul;
#pragma unroll
        for (int k = 0; k < 6; ++k) s[2 + k] += w * v[k];
      }
      if (ATOM) {
        const double eh = 0.5 * (evdwl + ecoul);
        ei += eh;
#pragma unroll
        for (int k = 0; k < 6; ++k) vi[k] += 0.5 * v[k];
        if (jw) {
          if (a.eatom) atomicAdd(&a.eatom[j], eh);
          if (a.vatom) {
#pragma unroll
            for (int k = 0; k < 6; ++k) atomicAdd(&a.vatom[6 * (size_t)j + k], 0.5 * v[k]);
          }
        }
      }
    }
  }
  fx = pair_wave_sum(fx); fy = pair_wave_sum(fy); fz = pair_wave_sum(fz);
  if (ATOM) {
    ei = pair_wave_sum(ei);
#pragma unroll
    for (int k = 0; k < 6; ++k) vi[k] = pair_wave_sum(vi[k]);
  }
  if (EV) {
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] = pair_wave_sum(s[k]);
  }
  if (lane != 0) return;
  if (jn > 0 && iw) {
    if (a.f) { atomicAdd(&a.f[3 * (size_t)i], fx); atomicAdd(&a.f[3 * (size_t)i + 1], fy); atomicAdd(&a.f[3 * (size_t)i + 2], fz); }
    if (ATOM) {
      if (a.eatom) atomicAdd(&a.eatom[i], ei);
      if (a.vatom) {
#pragma unroll
        for (int k = 0; k < 6; ++k) atomicAdd(&a.vatom[6 * (size_t)i + k], vi[k]);
      }
    }
  }
  if (EV) {
#pragma unroll
    for (int k = 0; k < 8; ++k) a.part[8 * (size_t)ii + k] = s[k];
  }
}

// ev[k] = sum over the rows of part[row][k], k < 8: every thread adds its rows in ascending order, then one fixed tree
__global__ __launch_bounds__(1024) void pair_finish_kernel(int nrows, const double *__restrict__ part, double *__restrict__ ev) {
#pragma clang fp contract(off)
  __shared__ double red[16][8];
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int r = threadIdx.x; r < nrows; r += 1024) {
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] += part[8 * (size_t)r + k];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = pair_wave_sum(s[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) red[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    double t = 0.0;
    for (int w = 0; w < 16; ++w) t += red[w][threadIdx.x];
    ev[threadIdx.x] = t;
  }
}

template <bool EV, bool ATOM>
void launch_pair_force_t(hipStream_t s, const PairArgs &a) {
  const dim3 grid((a.inum + 3) / 4), block(256);
  if (a.ntab <= PAIR_LDS_ENTRIES) hipLaunchKernelGGL((pair_force_kernel<EV, ATOM, true>), grid, block, 0, s, a);
  else hipLaunchKernelGGL((pair_force_kernel<EV, ATOM, false>), grid, block, 0, s, a);
}

}  // namespace

void launch_pair_pack(hipStream_t s, int nall, const double *x, const double *q, double4 *xq) {
  if (nall > 0) hipLaunchKernelGGL(pair_pack_kernel, dim3((nall + 255) / 256), dim3(256), 0, s, nall, x, q, xq);
}

void launch_pair_force(hipStream_t s, const PairArgs &a, double *ev) {
  const bool do_ev = ev != nullptr, do_atom = a.eatom != nullptr || a.vatom != nullptr;
  if (a.inum > 0) {
    if (do_ev && do_atom) launch_pair_force_t<true, true>(s, a);
    else if (do_ev) launch_pair_force_t<true, false>(s, a);
    else if (do_atom) launch_pair_force_t<false, true>(s, a);
    else launch_pair_force_t<false, false>(s, a);
  }
  if (do_ev) hipLaunchKernelGGL(pair_finish_kernel, dim3(1), dim3(1024), 0, s, a.inum, a.part, ev);
}

}  // namespace conp
