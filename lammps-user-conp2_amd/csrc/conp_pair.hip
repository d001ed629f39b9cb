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
//   pair_ordered_kernel  <EV, ATOM, LDS>: the atomic-free twin (section 26): one wavefront per receiving atom gathers its own row and
//                        its transposed entries (conp_transpose.hip); forces, eatom and vatom are bit-reproducible too.
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

// ---- the atomic-free twin (conp_pair_compute_ordered_device) ------------------------------------------------
// pair_force_kernel's pair body, operation for operation, as one function: fpair (and with E the two energies) of a pair at rsq whose
// table record is t, qi and qj in the OWNER's orientation (prefactor = qqrd2e qi qj / r).  false: outside cutsq, nothing is set.
template <bool E>
__device__ __forceinline__ bool pair_term(const PairArgs &a, const double *__restrict__ t, double qi, double qj, int sb, double rsq,
                                          double &fpair, double &evdwl, double &ecoul) {
#pragma clang fp contract(off)
  if (!(rsq < t[0])) return false;
  const double fc = a.special_coul[sb], fl = a.special_lj[sb];
  const double r2inv = 1.0 / rsq;
  double forcecoul = 0.0, forcelj = 0.0;
  ecoul = 0.0; evdwl = 0.0;
  if (rsq < a.cut_coulsq) {
    const double r = sqrt(rsq);
    const double grij = a.g_ewald * r;
    const double expm2 = exp(-grij * grij);
    const double tt = 1.0 / (1.0 + 0.3275911 * grij);
    const double erfc_ = tt * (0.254829592 + tt * (-0.284496736 + tt * (1.421413741 + tt * (-1.453152027 + tt * 1.061405429)))) * expm2;
    const double prefactor = a.qqrd2e * qi * qj / r;
    forcecoul = prefactor * (erfc_ + 1.12837917 * grij * expm2);
    if (fc < 1.0) forcecoul -= (1.0 - fc) * prefactor;
    if (E) {
      ecoul = prefactor * erfc_;
      if (fc < 1.0) ecoul -= (1.0 - fc) * prefactor;
    }
  }
  if (rsq < t[1]) {
    const double r6inv = r2inv * r2inv * r2inv;
    forcelj = r6inv * (t[2] * r6inv - t[3]);
    if (E) evdwl = fl * (r6inv * (t[4] * r6inv - t[5]) - t[6]);
  }
  fpair = (forcecoul + fl * forcelj) * r2inv;
  return true;
}

// One wavefront per atom `at` of [0, nall), four per workgroup.  The lanes stride first over at's own row (if own_row[at] >= 0): the
// pairs in which it is the i, with pair_force_kernel's lane assignment, so that the row's eight sums are that kernel's to the byte;
// then over at's transposed entries: the pairs in which it is the j, each in its OWNER's orientation (del = x_owner - x_at, types
// [type_owner][type_at]), of which at receives -(del fpair) and the owner's half of eatom / vatom.  An atom receives under
// newton || at < nlocal; an atom that cannot receive only records its row's sums (EV).  The wave's sums go through the fixed shuffle
// tree and lane 0 adds them with one plain read-add-write per output: no float atomic.  A row is written exactly when
// pair_force_kernel writes it: an own row with entries, or a transposed pair inside its cutoff.
template <bool EV, bool ATOM, bool LDS>
__global__ __launch_bounds__(256) void pair_ordered_kernel(PairArgs a, TransposedView tv) {
#pragma clang fp contract(off)
  __shared__ double tab_s[LDS ? PAIR_LDS_ENTRIES * PAIR_TAB_W : 1];
  const double *tab = a.tab;
  if (LDS) {
    for (int k = threadIdx.x; k < a.ntab * PAIR_TAB_W; k += 256) tab_s[k] = a.tab[k];
    __syncthreads();
    tab = tab_s;
  }
  const int at = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (at >= tv.nall) return;                     // (whole waves leave, after the only barrier)
  const int ii = tv.own_row[at];
  const bool recv = a.newton || at < a.nlocal;
  if (!recv && !(EV && ii >= 0)) return;
  const double4 pa = a.xq[at];
  const int ta = a.type[at];
  double fx = 0.0, fy = 0.0, fz = 0.0, ei = 0.0;
  double vi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  int jn = 0;
  if (ii >= 0) {                                 // the pairs in which `at` is the owner
    const int *jl = a.neigh + a.first[at];
    jn = a.numneigh[at];
    const int trow = ta * a.nt1;
    for (int jj = lane; jj < jn; jj += 64) {
      const int jraw = jl[jj];
      const int sb = (jraw >> 30) & 3, j = jraw & PAIR_MASK;
      const double4 pj = a.xq[j];
      const double delx = pa.x - pj.x, dely = pa.y - pj.y, delz = pa.z - pj.z;
      const double rsq = delx * delx + dely * dely + delz * delz;
      double fpair, evdwl, ecoul;
      if (!pair_term<EV || ATOM>(a, tab + (size_t)(trow + a.type[j]) * PAIR_TAB_W, pa.w, pj.w, sb, rsq, fpair, evdwl, ecoul)) continue;
      fx += delx * fpair; fy += dely * fpair; fz += delz * fpair;
      if (EV || ATOM) {
        const double v[6] = {delx * delx * fpair, dely * dely * fpair, delz * delz * fpair,
                             delx * dely * fpair, delx * delz * fpair, dely * delz * fpair};
        if (EV) {
          double w = 1.0;
          if (!a.newton) w = (at < a.nlocal ? 0.5 : 0.0) + (j < a.nlocal ? 0.5 : 0.0);
          s[0] += w * evdwl; s[1] += w * ecoul;
#pragma unroll
          for (int k = 0; k < 6; ++k) s[2 + k] += w * v[k];
        }
        if (ATOM) {
          ei += 0.5 * (evdwl + ecoul);
#pragma unroll
          for (int k = 0; k < 6; ++k) vi[k] += 0.5 * v[k];
        }
      }
    }
  }
  bool got = false;
  if (recv) {                                    // the pairs in which `at` is the j, ascending slot order
    const int lo = tv.tr_ptr[at], hi = tv.tr_ptr[at + 1];
    for (int k = lo + lane; k < hi; k += 64) {
      const int e = tv.tr_entry[k];
      const int sb = (e >> 30) & 3, i = e & PAIR_MASK;
      const double4 pi = a.xq[i];
      const double delx = pi.x - pa.x, dely = pi.y - pa.y, delz = pi.z - pa.z;
      const double rsq = delx * delx + dely * dely + delz * delz;
      double fpair, evdwl, ecoul;
      if (!pair_term<ATOM>(a, tab + (size_t)(a.type[i] * a.nt1 + ta) * PAIR_TAB_W, pi.w, pa.w, sb, rsq, fpair, evdwl, ecoul)) continue;
      got = true;
      fx += -(delx * fpair); fy += -(dely * fpair); fz += -(delz * fpair);
      if (ATOM) {
        ei += 0.5 * (evdwl + ecoul);
        vi[0] += 0.5 * (delx * delx * fpair); vi[1] += 0.5 * (dely * dely * fpair); vi[2] += 0.5 * (delz * delz * fpair);
        vi[3] += 0.5 * (delx * dely * fpair); vi[4] += 0.5 * (delx * delz * fpair); vi[5] += 0.5 * (dely * delz * fpair);
      }
    }
  }
  const bool any_tr = __ballot(got) != 0;
  const bool write = recv && (jn > 0 || any_tr);
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
  if (write) {
    if (a.f) {
      double *fa = a.f + 3 * (size_t)at;
      fa[0] = fa[0] + fx; fa[1] = fa[1] + fy; fa[2] = fa[2] + fz;
    }
    if (ATOM) {
      if (a.eatom) a.eatom[at] = a.eatom[at] + ei;
      if (a.vatom) {
#pragma unroll
        for (int k = 0; k < 6; ++k) a.vatom[6 * (size_t)at + k] = a.vatom[6 * (size_t)at + k] + vi[k];
      }
    }
  }
  if (EV && ii >= 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) a.part[8 * (size_t)ii + k] = s[k];
  }
}

template <bool EV, bool ATOM>
void launch_pair_ordered_t(hipStream_t s, const PairArgs &a, const TransposedView &t) {
  const dim3 grid((t.nall + 3) / 4), block(256);
  if (a.ntab <= PAIR_LDS_ENTRIES) hipLaunchKernelGGL((pair_ordered_kernel<EV, ATOM, true>), grid, block, 0, s, a, t);
  else hipLaunchKernelGGL((pair_ordered_kernel<EV, ATOM, false>), grid, block, 0, s, a, t);
}

}  // namespace

void launch_pair_force_ordered(hipStream_t s, const PairArgs &a, const TransposedView &t, double *ev) {
  const bool do_ev = ev != nullptr, do_atom = a.eatom != nullptr || a.vatom != nullptr;
  if (a.inum > 0 && t.nall > 0) {
    if (do_ev && do_atom) launch_pair_ordered_t<true, true>(s, a, t);
    else if (do_ev) launch_pair_ordered_t<true, false>(s, a, t);
    else if (do_atom) launch_pair_ordered_t<false, true>(s, a, t);
    else launch_pair_ordered_t<false, false>(s, a, t);
  }
  if (do_ev) hipLaunchKernelGGL(pair_finish_kernel, dim3(1), dim3(1024), 0, s, a.inum, a.part, ev);
}

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
