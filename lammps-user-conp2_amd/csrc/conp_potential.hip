// gfx950 kernels of the exact Ewald per-atom potential (conp_ewald_*, compute potential/atom without a mesh).
//
//   S_k = sum_j q_j e^{i k r_j} over every charged owned atom (electrolyte AND electrode), in G's (planar, kz) layout:
//     G[(p,a|b)][(m,c|s)] = sum_j q_j {cos,sin}(theta_pj) {cos,sin}(m uz z_j) = (Rp diag(q) Tz^T)[r][t]
//   g_i = - sum_{r,t} Rp[r][i] (w G)[r][t] Tz[t][i]     (the b vector's bilinear form, b_project_kernel, for any atom i)
//
// Atoms are taken in blocks: the phase tables of a block -- Rp [R_pad][nb_pad], Tz [C_pad][nb_pad], the electrode tables' layout --
// are made by conp_tables.hip's kernels from per-atom seeds that ew_seeds_kernel forms on the device (device sincos: the target is
// 1e-11 of the potential, not bit parity with libm).  Sources: ew_sk_kernel adds Rp diag(q) Tz^T of the block into split slices of
// G on the matrix cores; ew_sk_sum_kernel adds the slices in a fixed order.  Targets: b_project_kernel (conp_kernels.hip) with w o G;
// ew_out_kernel adds its four parts and scatters g_i, u_i to the atoms' local indices.
#include "conp_kernels.h"

namespace conp {

typedef double d4 __attribute__((ext_vector_type(4)));
#define MFMA_F64(a, b, c) __builtin_amdgcn_mfma_f64_16x16x4f64((a), (b), (c), 0, 0, 0)

// seeds[6][n] = (cos, sin)(unitk_c x_ic), c = x, y, z: what electrode_seeds makes on the host for the electrode tables
__global__ __launch_bounds__(256) void ew_seeds_kernel(int n, const double *__restrict__ x, double ux, double uy, double uz,
                                                       double *__restrict__ seeds) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double u[3] = {ux, uy, uz};
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    double s, co;
    sincos(u[c] * x[3 * (size_t)i + c], &s, &co);
    seeds[(size_t)(2 * c) * n + i] = co;
    seeds[(size_t)(2 * c + 1) * n + i] = s;
  }
}

// Gp[z][r][t] += sum_{j in split z} Rp[r][j] q[j] Tz[t][j] for one block of atoms.  Workgroup: one row tile (128 G rows) x 64 G
// columns, four waves of 64 x 32 (4 x 2 fragments); the atoms of its split in chunks of 16, staged through LDS (16 consecutive atoms
// of a row = one 128-byte read).  Column chunks past the sphere cut of the row tile (KPlan::nba_rc) are skipped: their w is zero,
// and their G stays zero.  Split z owns slice z: blocks are added by successive launches, no two workgroups write one entry.
__global__ __launch_bounds__(256) void ew_sk_kernel(int C_pad, int n_row_tiles, int nb_pad, int per_split, const int *__restrict__ nb_act,
                                                    const double *__restrict__ Rp, const double *__restrict__ Tz,
                                                    const double *__restrict__ q, double *__restrict__ Gp, size_t slice) {
  __shared__ double sa[128][17];
  __shared__ double sb[64][17];
  const int rt = blockIdx.y, c0 = 64 * blockIdx.x;
  const int ct = c0 / 320, blk = (c0 - 320 * ct) / 32;
  if (blk >= nb_act[ct * n_row_tiles + rt]) return;                 // (uniform over the workgroup, before any barrier)
  const int j_lo = blockIdx.z * per_split, j_hi = min(nb_pad, j_lo + per_split);
  if (j_lo >= j_hi) return;
  const int r0 = 128 * rt;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  const int wr = 64 * (wave >> 1), wc = 32 * (wave & 1);
  d4 acc[4][2];
#pragma unroll
  for (int f = 0; f < 4; ++f)
#pragma unroll
    for (int g = 0; g < 2; ++g) acc[f][g] = (d4){0.0, 0.0, 0.0, 0.0};
  for (int j0 = j_lo; j0 < j_hi; j0 += 16) {
    __syncthreads();
    for (int e = t; e < 128 * 16; e += 256) {
      const int r = e >> 4, a = e & 15;
      sa[r][a] = Rp[(size_t)(r0 + r) * nb_pad + j0 + a];
    }
    for (int e = t; e < 64 * 16; e += 256) {
      const int c = e >> 4, a = e & 15;
      sb[c][a] = Tz[(size_t)(c0 + c) * nb_pad + j0 + a] * q[j0 + a];
    }
    __syncthreads();
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
      double af[4], bf[2];
#pragma unroll
      for (int f = 0; f < 4; ++f) af[f] = sa[wr + 16 * f + fr][4 * ks + fk];
#pragma unroll
      for (int g = 0; g < 2; ++g) bf[g] = sb[wc + 16 * g + fr][4 * ks + fk];
#pragma unroll
      for (int f = 0; f < 4; ++f)
#pragma unroll
        for (int g = 0; g < 2; ++g) acc[f][g] = MFMA_F64(af[f], bf[g], acc[f][g]);
    }
  }
  double *out = Gp + slice * blockIdx.z;
#pragma unroll
  for (int f = 0; f < 4; ++f)
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        out[(size_t)(r0 + wr + 16 * f + fk + 4 * r) * C_pad + c0 + wc + 16 * g + fr] += acc[f][g][r];
}

// G = sum over the slices, in slice order
__global__ __launch_bounds__(256) void ew_sk_sum_kernel(size_t n, int nsplit, const double *__restrict__ Gp, double *__restrict__ G) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= n) return;
  double s = Gp[e];
  for (int z = 1; z < nsplit; ++z) s += Gp[(size_t)z * n + e];
  G[e] = s;
}

// w o G in b_project_kernel's fragment-major order: Gwf[((rf (C_pad/4)) + ts) 64 + 16 fk + fr] = (w G)[16 rf + fr][4 ts + fk]
__global__ __launch_bounds__(256) void ew_gw_kernel(int R_pad, int C_pad, const double *__restrict__ wfull, const double *__restrict__ G,
                                                    double *__restrict__ Gwf) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)R_pad * C_pad) return;
  const int r = (int)(e / C_pad), c = (int)(e - (size_t)r * C_pad);
  Gwf[((size_t)(r >> 4) * (C_pad / 4) + (c >> 2)) * 64 + 16 * (c & 3) + (r & 15)] = wfull[e] * G[e];
}

// the four parts of b_project_kernel in its fixed order, scattered to the targets' local indices
__global__ __launch_bounds__(256) void ew_out_kernel(int n, int nb_pad, const double *__restrict__ bk, const int *__restrict__ idx,
                                                     const double *__restrict__ q, double selfc, double *__restrict__ g_out,
                                                     double *__restrict__ u_out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double g = (bk[i] + bk[(size_t)nb_pad + i]) + (bk[2 * (size_t)nb_pad + i] + bk[3 * (size_t)nb_pad + i]);
  g_out[idx[i]] = g;
  u_out[idx[i]] = g + selfc * q[i];
}

void launch_ew_seeds(hipStream_t s, int n, const double *x, double ux, double uy, double uz, double *seeds) {
  if (n <= 0) return;
  hipLaunchKernelGGL(ew_seeds_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, x, ux, uy, uz, seeds);
}

void launch_ew_sk(hipStream_t s, const DevPlan &pl, int nb_pad, int nsplit, const double *Rp, const double *Tz, const double *q,
                  double *Gp) {
  const int per_split = ((nb_pad + nsplit - 1) / nsplit + 15) / 16 * 16;
  hipLaunchKernelGGL(ew_sk_kernel, dim3(pl.C_pad / 64, pl.n_row_tiles, nsplit), dim3(256), 0, s, pl.C_pad, pl.n_row_tiles, nb_pad,
                     per_split, pl.nb_act, Rp, Tz, q, Gp, (size_t)pl.R_pad * pl.C_pad);
}

void launch_ew_sk_sum(hipStream_t s, const DevPlan &pl, int nsplit, const double *Gp, double *G) {
  const size_t n = (size_t)pl.R_pad * pl.C_pad;
  hipLaunchKernelGGL(ew_sk_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n, nsplit, Gp, G);
}

void launch_ew_gw(hipStream_t s, const DevPlan &pl, const double *G, double *Gwf) {
  const size_t n = (size_t)pl.R_pad * pl.C_pad;
  hipLaunchKernelGGL(ew_gw_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pl.R_pad, pl.C_pad, pl.wfull, G, Gwf);
}

void launch_ew_out(hipStream_t s, int n, int nb_pad, const double *bk, const int *idx, const double *q, double selfc, double *g_out,
                   double *u_out) {
  if (n <= 0) return;
  hipLaunchKernelGGL(ew_out_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, nb_pad, bk, idx, q, selfc, g_out, u_out);
}

}  // namespace conp
