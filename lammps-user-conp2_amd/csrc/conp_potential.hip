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
// The reciprocal-space forces, energy and virial (conp_ewald_compute_forces) are the same projection with its
// derivatives: ew_force_kernel, ew_energy_virial_kernel, ew_force_out_kernel below.
#include "conp_kernels.h"
#include <algorithm>

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

// ---- exact Ewald forces, energy and virial (conp_ewald_compute_forces) ---------------------------------------
// At fixed S the force on atom i is qqrd2e q_i grad g_i: the gradient of b_project_kernel's bilinear form through the atom's own
// phase columns.  d/dx and d/dy act on Rp (d cos theta = -k sin theta, d sin theta = k cos theta: a row's derivative is its (a, b)
// partner row -- 64 rows away in the row tile -- times -+ k_x or k_y of the planar vector); d/dz acts on Tz (a column's derivative is
// its (c, s) partner column -- 8 columns away in the 16-column fragment -- times -+ k_z of the column):
//     H  = (w G) Tz          g     = - sum_r Rp[r] H[r]
//     Hz = (w G) dTz/dz      dg/dz = - sum_r Rp[r] Hz[r]
//     dg/dx = - sum_r s_r kx_r Rp[r ^ 64] H[r]   (s_r = -1 on 'a' rows, +1 on 'b' rows), dg/dy likewise with ky_r = sgn ky
// ew_force_kernel is b_project_kernel with a second accumulator set: the (w G) fragments are read once and feed both products; the
// B operands of Hz are the staged Tz values of the partner k-step (k-step i ^ 2 of a group of eight: 4 columns per k-step), scaled
// in registers.  Units and parts are b_project_kernel's; the two accumulator sets and the sixteen running sums of a lane take twice
// its registers, so a workgroup is 8 waves (256 registers each) where b_project_kernel has 16: a part's units are dealt to 8 waves.
// out[(4 quantity + part) ne_pad + i], quantity = g, dg/dx, dg/dy, dg/dz
__global__ __launch_bounds__(512) void ew_force_kernel(int C_pad, int ne_pad, int n_col_tiles, int kzt, double ux, double uy, double uz,
                                                        const int *__restrict__ ct_ptr, const SkTile *__restrict__ tiles,
                                                        const int *__restrict__ p_ikx, const int *__restrict__ p_iky,
                                                        const int *__restrict__ p_sgn, const double *__restrict__ Gwf,
                                                        const double *__restrict__ Rp, const double *__restrict__ Tz,
                                                        double *__restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double *tz = reinterpret_cast<double *>(smem);          // [4 atom fragments][160 columns][16 atoms]
  double *red = tz + 4 * 160 * 16;                         // [4 quantities][8 waves][64]
  const int part = blockIdx.y;
  const int i0 = blockIdx.x * 64;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  double psum[4][4];
#pragma unroll
  for (int v = 0; v < 4; ++v)
#pragma unroll
    for (int c = 0; c < 4; ++c) psum[v][c] = 0.0;
  for (int ct = 0; ct < n_col_tiles; ++ct) {
    const int tb = ct_ptr[ct], te = ct_ptr[ct + 1];
    if (te <= tb) continue;
    int nba_max = 0;
    for (int k = tb; k < te; ++k) nba_max = tiles[k].nba > nba_max ? tiles[k].nba : nba_max;
    for (int h = 0; h < 2; ++h) {                        // columns [160 h, 160 h + 160) of the tile = k-steps [40 h, 40 h + 40)
      if (40 * h >= 8 * nba_max) break;
      __syncthreads();
      for (int e = t; e < 160 * 64; e += 512) {
        const int col = e >> 6, a = e & 63;
        tz[((a >> 4) * 160 + col) * 16 + (a & 15)] = Tz[(size_t)(ct * 320 + 160 * h + col) * ne_pad + i0 + a];
      }
      __syncthreads();
      const int nu = 8 * (te - tb);
      for (int u = part + 4 * wave; u < nu; u += 32) {
        const SkTile tl = tiles[tb + (u >> 3)];
        const int rf = tl.rt * 8 + (u & 7);
        const int ks0 = 40 * h, ks1 = 8 * tl.nba < 40 * (h + 1) ? 8 * tl.nba : 40 * (h + 1);
        if (ks1 <= ks0) continue;
        d4 acc[4], accz[4];
#pragma unroll
        for (int c = 0; c < 4; ++c) { acc[c] = (d4){0.0, 0.0, 0.0, 0.0}; accz[c] = (d4){0.0, 0.0, 0.0, 0.0}; }
        const double *ap = Gwf + ((size_t)rf * (C_pad / 4) + (size_t)ct * 80) * 64 + lane;
        const double *bp = tz + fk * 16 + fr;
        double an[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) an[i] = ap[(size_t)(ks0 + i) * 64];
#pragma unroll 1
        for (int tg = ks0; tg < ks1; tg += 8) {
          double ac[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) ac[i] = an[i];
          if (tg + 8 < ks1) {
#pragma unroll
            for (int i = 0; i < 8; ++i) an[i] = ap[(size_t)(tg + 8 + i) * 64];
          }
          const double *bq = bp + 64 * (tg - ks0);
          // k-step tg + i holds the tile's columns 4 (tg + i) + fk: fragment 2 (tg / 8) + (i >> 2), cos columns for i & 2 == 0,
          // kz index (within the fragment) 4 (i & 1) + fk
          const double kz0 = uz * (double)(ct * kzt + 2 * tg + fk);
          double b[8][4];
#pragma unroll
          for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) b[i][c] = bq[64 * i + c * 160 * 16];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const double kz = kz0 + uz * (double)(8 * (i >> 2) + 4 * (i & 1));
            const double sk = (i & 2) ? kz : -kz;          // d cos = -kz sin, d sin = kz cos
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              acc[c] = MFMA_F64(ac[i], b[i][c], acc[c]);
              accz[c] = MFMA_F64(ac[i], sk * b[i ^ 2][c], accz[c]);
            }
          }
        }
        const bool brow = (u & 4) != 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * rf + fk + 4 * r;
          const int p = 64 * tl.rt + 16 * (u & 3) + fk + 4 * r;
          const double sg = brow ? 1.0 : -1.0;
          const double kx = sg * ux * (double)p_ikx[p], ky = sg * uy * (double)(p_sgn[p] * p_iky[p]);
          const double *rp = Rp + (size_t)row * ne_pad + i0 + fr;
          const double *rq = Rp + (size_t)(row ^ 64) * ne_pad + i0 + fr;
#pragma unroll
          for (int c = 0; c < 4; ++c) {
            const double own = rp[16 * c], oth = rq[16 * c] * acc[c][r];
            psum[0][c] += own * acc[c][r];
            psum[1][c] += kx * oth;
            psum[2][c] += ky * oth;
            psum[3][c] += own * accz[c][r];
          }
        }
      }
    }
  }
#pragma unroll
  for (int v = 0; v < 4; ++v)
#pragma unroll
    for (int c = 0; c < 4; ++c) { psum[v][c] += __shfl_xor(psum[v][c], 16, 64); psum[v][c] += __shfl_xor(psum[v][c], 32, 64); }
  __syncthreads();
  if (lane < 16) {
#pragma unroll
    for (int v = 0; v < 4; ++v)
#pragma unroll
      for (int c = 0; c < 4; ++c) red[(v * 8 + wave) * 64 + 16 * c + lane] = psum[v][c];
  }
  __syncthreads();
  if (t < 256) {
    const int v = t >> 6, a = t & 63;
    double sum = 0.0;
    for (int w = 0; w < 8; ++w) sum += red[(v * 8 + w) * 64 + a];
    out[(size_t)(4 * v + part) * ne_pad + i0 + a] = -sum;
  }
}

// The seven k-sums of the energy and the virial from G: per listed k (the reference's half list) |S_k|^2 from the four entries
// sfac_gather_kernel reads, e_k = ug_k |S_k|^2, v_ab = e_k (delta_ab - 2 (1 / k^2 + 1 / (4 g^2)) k_a k_b).  Thread t of workgroup b
// adds the terms k = 256 b + t, + 256 gridDim.x, ... in that order, the workgroup adds its threads in a binary tree, and the last
// launch (final = 1, one workgroup) adds the workgroups' rows the same way: a fixed order for a given K.
// kv: [4][K] = ug, kx, ky, kz.  part: [gridDim.x][7] = sum e, xx, yy, zz, xy, xz, yz
__global__ __launch_bounds__(256) void ew_energy_virial_kernel(int K, int C_pad, int PT, const int *__restrict__ row_a,
                                                               const int *__restrict__ col_c, const int *__restrict__ k_sign,
                                                               const double *__restrict__ kv, double inv4g2, const double *__restrict__ G,
                                                               const double *__restrict__ in, int nin, double *__restrict__ part,
                                                               int final) {
  __shared__ double sh[7][256];
  const int t = threadIdx.x;
  double a[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (final) {
    for (int j = t; j < nin; j += 256)
#pragma unroll
      for (int v = 0; v < 7; ++v) a[v] += in[(size_t)j * 7 + v];
  } else {
    for (int k = blockIdx.x * 256 + t; k < K; k += 256 * gridDim.x) {
      const size_t ra = (size_t)row_a[k] * C_pad, rb = (size_t)(row_a[k] + PT) * C_pad;
      const int cc = col_c[k], cs = col_c[k] + 8;
      const double CC = G[ra + cc], CS = G[ra + cs], SC = G[rb + cc], SS = G[rb + cs];
      const double sg = (double)k_sign[k];
      const double sr = CC - sg * SS, si = SC + sg * CS;
      const double kx = kv[(size_t)K + k], ky = kv[2 * (size_t)K + k], kz = kv[3 * (size_t)K + k];
      const double e = kv[k] * (sr * sr + si * si);
      const double vt = -2.0 * (1.0 / (kx * kx + ky * ky + kz * kz) + inv4g2) * e;
      a[0] += e;
      a[1] += e + vt * kx * kx; a[2] += e + vt * ky * ky; a[3] += e + vt * kz * kz;
      a[4] += vt * kx * ky; a[5] += vt * kx * kz; a[6] += vt * ky * kz;
    }
  }
#pragma unroll
  for (int v = 0; v < 7; ++v) sh[v][t] = a[v];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s)
#pragma unroll
      for (int v = 0; v < 7; ++v) sh[v][t] += sh[v][t + s];
    __syncthreads();
  }
  if (t < 7) part[(size_t)blockIdx.x * 7 + t] = sh[t][0];
}

// the four parts of ew_force_kernel's four quantities in b_project's fixed order; force (with the slab term), per-atom energy,
// scattered to the targets' local indices.  fo: [nlocal][3] and eo: [nlocal], overwritten at idx (the host accumulates).
// DEV (the device-resident entry): atom i of the block is atom base + i itself, Q, M, M2 are read from `four`, fo is added to
template <bool DEV>
__global__ __launch_bounds__(256) void ew_force_out_kernel(int n, int nb_pad, const double *__restrict__ bk, const int *__restrict__ idx,
                                                           const double *__restrict__ q, const double *__restrict__ x, EwForceOut o,
                                                           const double *__restrict__ four, int base, double *__restrict__ fo,
                                                           double *__restrict__ eo) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  double v[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) {
    const double *b = bk + (size_t)(4 * c) * nb_pad + i;
    v[c] = (b[0] + b[(size_t)nb_pad]) + (b[2 * (size_t)nb_pad] + b[3 * (size_t)nb_pad]);
  }
  const double qi = q[i];
  if (DEV)
    kspace_atom_out<true>(kspace_out_from_sums(o, four), qi, x[3 * (size_t)i + 2], v[0], qi * v[1], qi * v[2], qi * v[3],
                          (size_t)base + i, fo, eo);
  else
    kspace_atom_out(o, qi, x[3 * (size_t)i + 2], v[0], qi * v[1], qi * v[2], qi * v[3], (size_t)idx[i], fo, eo);
}

// Q, Q2, M, M2 over the atoms [0, n) (zero charges add exact zeros) in ew_energy_virial_kernel's scheme: thread t of workgroup b
// adds the atoms 256 b + t, + 256 gridDim.x, ... in that order, the workgroup adds its threads in a binary tree, and the last launch
// (final = 1, one workgroup) adds the workgroups' rows the same way: a fixed order for a given n, no atomics.  part: [gridDim.x][4]
__global__ __launch_bounds__(256) void kspace_four_sums_kernel(int n, const double *__restrict__ x, const double *__restrict__ q,
                                                               const double *__restrict__ in, int nin, double *__restrict__ part,
                                                               int final) {
  __shared__ double sh[4][256];
  const int t = threadIdx.x;
  double a[4] = {0.0, 0.0, 0.0, 0.0};
  if (final) {
    for (int j = t; j < nin; j += 256)
#pragma unroll
      for (int v = 0; v < 4; ++v) a[v] += in[(size_t)j * 4 + v];
  } else {
    for (int i = blockIdx.x * 256 + t; i < n; i += 256 * gridDim.x) {
      const double qi = q[i], z = x[3 * (size_t)i + 2];
      a[0] += qi; a[1] += qi * qi; a[2] += qi * z; a[3] += qi * z * z;
    }
  }
#pragma unroll
  for (int v = 0; v < 4; ++v) sh[v][t] = a[v];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if (t < s)
#pragma unroll
      for (int v = 0; v < 4; ++v) sh[v][t] += sh[v][t + s];
    __syncthreads();
  }
  if (t < 4) part[(size_t)blockIdx.x * 4 + t] = sh[t][0];
}

// ev[0] = qs (s7[0] - g Q2 / sqrt(pi) - (pi / 2) Q^2 / (g^2 V) [+ 2 pi (M^2 - Q M2 - Q^2 L^2 / 12) / V]), ev[1 + c] = qs s7[1 + c]:
// the host entries' expressions, one lane per output
__global__ __launch_bounds__(64) void kspace_finish_kernel(KspaceFinish a, const double *__restrict__ s7, const double *__restrict__ four,
                                                          double *__restrict__ ev) {
#pragma clang fp contract(off)
  const int t = threadIdx.x;
  if (t >= 7) return;
  double v = s7[t];
  if (t == 0) {
    const double Q = four[0], Q2 = four[1], M = four[2], M2 = four[3];
    v = v - a.g_pis * Q2 - a.qcoef * Q * Q;
    if (a.slab) v += a.slab_pref * (M * M - Q * M2 - Q * Q * a.L2_12);
  }
  ev[t] = a.qs * v;
}

// ---- per-atom virial of the exact Ewald sum (conp_ewald_compute_forces_vatom) -------------------------------
// vatom_i,ab = qs q_i sum_k ug_k (delta_ab - 2 c_k k_a k_b) A_i(k), c_k = 1 / k^2 + 1 / (4 g^2).  The delta part is -g_i / 2 (the force
// kernel's first quantity).  The k_a k_b part, KK_ab = sum_k 2 ug_k c_k k_a k_b A_i(k), is minus the Hessian at fixed S of the
// projection with the second weight set w' = c o w:
//     H' = (w' G) Tz       KK_xx, KK_yy, KK_xy = sum_r (kx_r^2, ky_r^2, kx_r ky_r) Rp[r] H'[r]
//     H'zz = (w' G) (kz^2 Tz)                      KK_zz = sum_r Rp[r] H'zz[r]
//     H'z = (w' G) dTz/dz   KK_xz, KK_yz = - sum_r s_r (kx_r, ky_r) Rp[r ^ 64] H'z[r]     (ew_force_kernel's partner rows and columns)

// (c o w) o G in ew_gw_kernel's order; c of entry (r, t) from the planar vector of row r and the kz index of column t
__global__ __launch_bounds__(256) void ew_gw2_kernel(int R_pad, int C_pad, int kzt, double ux, double uy, double uz, double inv4g2,
                                                     const int *__restrict__ p_ikx, const int *__restrict__ p_iky,
                                                     const double *__restrict__ wfull, const double *__restrict__ G,
                                                     double *__restrict__ Gwf2) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)R_pad * C_pad) return;
  const int r = (int)(e / C_pad), c = (int)(e - (size_t)r * C_pad);
  const double w = wfull[e];
  double v = 0.0;
  if (w != 0.0) {
    const int p = 64 * (r >> 7) + (r & 63);
    const int ct = c / 320, cl = c - 320 * ct, m = ct * kzt + 8 * (cl >> 4) + (cl & 7);
    const double kx = ux * (double)p_ikx[p], ky = uy * (double)p_iky[p], kz = uz * (double)m;
    v = w * (1.0 / (kx * kx + ky * ky + kz * kz) + inv4g2) * G[e];
  }
  Gwf2[((size_t)(r >> 4) * (C_pad / 4) + (c >> 2)) * 64 + 16 * (c & 3) + (r & 15)] = v;
}

// ew_force_kernel's loop with the chains above, in two passes so that a pass holds at most two accumulator sets and four running
// sums per atom fragment (the force kernel's register budget, no scratch):
//   PASS 0: H' and H'zz -> out quantities 0..3 = KK_xx, KK_yy, KK_xy, KK_zz        PASS 1: H'z -> out quantities 4, 5 = KK_xz, KK_yz
// out[(4 quantity + part) ne_pad + i]; units, parts and the order of every sum are ew_force_kernel's
template <int PASS>
__global__ __launch_bounds__(512) void ew_vatom_kernel(int C_pad, int ne_pad, int n_col_tiles, int kzt, double ux, double uy, double uz,
                                                        const int *__restrict__ ct_ptr, const SkTile *__restrict__ tiles,
                                                        const int *__restrict__ p_ikx, const int *__restrict__ p_iky,
                                                        const int *__restrict__ p_sgn, const double *__restrict__ Gwf2,
                                                        const double *__restrict__ Rp, const double *__restrict__ Tz,
                                                        double *__restrict__ out) {
  constexpr int NQ = PASS == 0 ? 4 : 2;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  double *tz = reinterpret_cast<double *>(smem);          // [4 atom fragments][160 columns][16 atoms]
  double *red = tz + 4 * 160 * 16;                         // [NQ quantities][8 waves][64]
  const int part = blockIdx.y;
  const int i0 = blockIdx.x * 64;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const int fr = lane & 15, fk = lane >> 4;
  double psum[NQ][4];
#pragma unroll
  for (int v = 0; v < NQ; ++v)
#pragma unroll
    for (int c = 0; c < 4; ++c) psum[v][c] = 0.0;
  for (int ct = 0; ct < n_col_tiles; ++ct) {
    const int tb = ct_ptr[ct], te = ct_ptr[ct + 1];
    if (te <= tb) continue;
    int nba_max = 0;
    for (int k = tb; k < te; ++k) nba_max = tiles[k].nba > nba_max ? tiles[k].nba : nba_max;
    for (int h = 0; h < 2; ++h) {                        // columns [160 h, 160 h + 160) of the tile = k-steps [40 h, 40 h + 40)
      if (40 * h >= 8 * nba_max) break;
      __syncthreads();
      for (int e = t; e < 160 * 64; e += 512) {
        const int col = e >> 6, a = e & 63;
        tz[((a >> 4) * 160 + col) * 16 + (a & 15)] = Tz[(size_t)(ct * 320 + 160 * h + col) * ne_pad + i0 + a];
      }
      __syncthreads();
      const int nu = 8 * (te - tb);
      for (int u = part + 4 * wave; u < nu; u += 32) {
        const SkTile tl = tiles[tb + (u >> 3)];
        const int rf = tl.rt * 8 + (u & 7);
        const int ks0 = 40 * h, ks1 = 8 * tl.nba < 40 * (h + 1) ? 8 * tl.nba : 40 * (h + 1);
        if (ks1 <= ks0) continue;
        d4 acc[4], accz[4];                               // PASS 0: H', H'zz.  PASS 1: accz = H'z (acc unused)
#pragma unroll
        for (int c = 0; c < 4; ++c) { acc[c] = (d4){0.0, 0.0, 0.0, 0.0}; accz[c] = (d4){0.0, 0.0, 0.0, 0.0}; }
        const double *ap = Gwf2 + ((size_t)rf * (C_pad / 4) + (size_t)ct * 80) * 64 + lane;
        const double *bp = tz + fk * 16 + fr;
        double an[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) an[i] = ap[(size_t)(ks0 + i) * 64];
#pragma unroll 1
        for (int tg = ks0; tg < ks1; tg += 8) {
          double ac[8];
#pragma unroll
          for (int i = 0; i < 8; ++i) ac[i] = an[i];
          if (tg + 8 < ks1) {
#pragma unroll
            for (int i = 0; i < 8; ++i) an[i] = ap[(size_t)(tg + 8 + i) * 64];
          }
          const double *bq = bp + 64 * (tg - ks0);
          const double kz0 = uz * (double)(ct * kzt + 2 * tg + fk);      // (ew_force_kernel: the kz of k-step tg + i)
          double b[8][4];
#pragma unroll
          for (int i = 0; i < 8; ++i)
#pragma unroll
            for (int c = 0; c < 4; ++c) b[i][c] = bq[64 * i + c * 160 * 16];
#pragma unroll
          for (int i = 0; i < 8; ++i) {
            const double kz = kz0 + uz * (double)(8 * (i >> 2) + 4 * (i & 1));
            if (PASS == 0) {
              const double kz2 = kz * kz;
#pragma unroll
              for (int c = 0; c < 4; ++c) {
                acc[c] = MFMA_F64(ac[i], b[i][c], acc[c]);
                accz[c] = MFMA_F64(ac[i], kz2 * b[i][c], accz[c]);
              }
            } else {
              const double sk = (i & 2) ? kz : -kz;        // d cos = -kz sin, d sin = kz cos
#pragma unroll
              for (int c = 0; c < 4; ++c) accz[c] = MFMA_F64(ac[i], sk * b[i ^ 2][c], accz[c]);
            }
          }
        }
        const bool brow = (u & 4) != 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * rf + fk + 4 * r;
          const int p = 64 * tl.rt + 16 * (u & 3) + fk + 4 * r;
          const double kx = ux * (double)p_ikx[p], ky = uy * (double)(p_sgn[p] * p_iky[p]);
          if (PASS == 0) {
            const double *rp = Rp + (size_t)row * ne_pad + i0 + fr;
            const double kxx = kx * kx, kyy = ky * ky, kxy = kx * ky;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const double own = rp[16 * c], hv = own * acc[c][r];
              psum[0][c] += kxx * hv;
              psum[1][c] += kyy * hv;
              psum[2][c] += kxy * hv;
              psum[3][c] += own * accz[c][r];
            }
          } else {
            const double sg = brow ? 1.0 : -1.0;
            const double *rq = Rp + (size_t)(row ^ 64) * ne_pad + i0 + fr;
#pragma unroll
            for (int c = 0; c < 4; ++c) {
              const double oth = rq[16 * c] * accz[c][r];
              psum[0][c] += sg * kx * oth;
              psum[1][c] += sg * ky * oth;
            }
          }
        }
      }
    }
  }
#pragma unroll
  for (int v = 0; v < NQ; ++v)
#pragma unroll
    for (int c = 0; c < 4; ++c) { psum[v][c] += __shfl_xor(psum[v][c], 16, 64); psum[v][c] += __shfl_xor(psum[v][c], 32, 64); }
  __syncthreads();
  if (lane < 16) {
#pragma unroll
    for (int v = 0; v < NQ; ++v)
#pragma unroll
      for (int c = 0; c < 4; ++c) red[(v * 8 + wave) * 64 + 16 * c + lane] = psum[v][c];
  }
  __syncthreads();
  if (t < 64 * NQ) {
    const int v = t >> 6, a = t & 63;
    double sum = 0.0;
    for (int w = 0; w < 8; ++w) sum += red[(v * 8 + w) * 64 + a];
    out[(size_t)(4 * ((PASS == 0 ? 0 : 4) + v) + part) * ne_pad + i0 + a] = PASS == 0 ? sum : -sum;
  }
}

// vo[a][6] = qs q_i (delta_ab (-g_i / 2) - KK_ab) in the order xx, yy, zz, xy, xz, yz: g_i from the force kernel's first quantity
// (bk), KK from ew_vatom_kernel (vk: xx, yy, xy, zz, xz, yz), each the four parts in b_project's fixed order.  A zero charge writes
// exact zeros.  DEV: atom i of the block is atom base + i itself; else scattered to idx
template <bool DEV>
__global__ __launch_bounds__(256) void ew_vatom_out_kernel(int n, int nb_pad, const double *__restrict__ bk, const double *__restrict__ vk,
                                                           const int *__restrict__ idx, const double *__restrict__ q, double qs, int base,
                                                           double *__restrict__ vo) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double g = (bk[i] + bk[(size_t)nb_pad + i]) + (bk[2 * (size_t)nb_pad + i] + bk[3 * (size_t)nb_pad + i]);
  double kk[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    const double *b = vk + (size_t)(4 * c) * nb_pad + i;
    kk[c] = (b[0] + b[(size_t)nb_pad]) + (b[2 * (size_t)nb_pad] + b[3 * (size_t)nb_pad]);
  }
  const double qi = q[i], d = -0.5 * g;
  double *v = vo + 6 * (DEV ? (size_t)base + i : (size_t)idx[i]);
  if (qi == 0.0) {
#pragma unroll
    for (int c = 0; c < 6; ++c) v[c] = 0.0;
    return;
  }
  const double s = qs * qi;
  v[0] = s * (d - kk[0]); v[1] = s * (d - kk[1]); v[2] = s * (d - kk[3]);
  v[3] = s * (-kk[2]); v[4] = s * (-kk[4]); v[5] = s * (-kk[5]);
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

void launch_ew_force(hipStream_t s, const DevPlan &pl, int kzt, double ux, double uy, double uz, int nb_pad, const int *ct_ptr,
                     const SkTile *tiles, const double *Gwf, const double *Rp, const double *Tz, double *out) {
  const size_t lds = ((size_t)4 * 160 * 16 + 4 * 8 * 64) * sizeof(double);
  static DynLdsCache granted{};
  ensure_dyn_lds(ew_force_kernel, lds, granted);
  hipLaunchKernelGGL(ew_force_kernel, dim3(nb_pad / 64, 4), dim3(512), lds, s, pl.C_pad, nb_pad, pl.n_col_tiles, kzt, ux, uy, uz, ct_ptr,
                     tiles, pl.p_ikx, pl.p_iky, pl.p_sgn, Gwf, Rp, Tz, out);
}

int ew_energy_virial_workgroups(int K) { return std::max(1, std::min(256, (K + 255) / 256)); }

void launch_ew_energy_virial(hipStream_t s, int K, int C_pad, int PT, const int *sf_row_a, const int *sf_col_c, const int *k_sign,
                             const double *kv, double g_ewald, const double *G, double *part, double *sums) {
  const int nwg = ew_energy_virial_workgroups(K);
  const double inv4g2 = 1.0 / (4.0 * g_ewald * g_ewald);
  hipLaunchKernelGGL(ew_energy_virial_kernel, dim3(nwg), dim3(256), 0, s, K, C_pad, PT, sf_row_a, sf_col_c, k_sign, kv, inv4g2, G,
                     (const double *)nullptr, 0, part, 0);
  hipLaunchKernelGGL(ew_energy_virial_kernel, dim3(1), dim3(256), 0, s, K, C_pad, PT, sf_row_a, sf_col_c, k_sign, kv, inv4g2, G,
                     (const double *)part, nwg, sums, 1);
}

void launch_ew_force_out(hipStream_t s, int n, int nb_pad, const double *bk, const int *idx, const double *q, const double *x,
                         const EwForceOut &o, double *fo, double *eo) {
  if (n <= 0) return;
  hipLaunchKernelGGL(ew_force_out_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, s, n, nb_pad, bk, idx, q, x, o,
                     (const double *)nullptr, 0, fo, eo);
}

void launch_ew_force_out_device(hipStream_t s, int n, int nb_pad, const double *bk, const double *q, const double *x, const EwForceOut &o,
                                const double *four, int base, double *fo, double *eo) {
  if (n <= 0) return;
  hipLaunchKernelGGL(ew_force_out_kernel<true>, dim3((n + 255) / 256), dim3(256), 0, s, n, nb_pad, bk, (const int *)nullptr, q, x, o,
                     four, base, fo, eo);
}

void launch_ew_gw2(hipStream_t s, const DevPlan &pl, int kzt, double ux, double uy, double uz, double g_ewald, const double *G,
                   double *Gwf2) {
  const size_t n = (size_t)pl.R_pad * pl.C_pad;
  hipLaunchKernelGGL(ew_gw2_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pl.R_pad, pl.C_pad, kzt, ux, uy, uz,
                     1.0 / (4.0 * g_ewald * g_ewald), pl.p_ikx, pl.p_iky, pl.wfull, G, Gwf2);
}

void launch_ew_vatom(hipStream_t s, const DevPlan &pl, int kzt, double ux, double uy, double uz, int nb_pad, const int *ct_ptr,
                     const SkTile *tiles, const double *Gwf2, const double *Rp, const double *Tz, double *out) {
  const size_t lds = ((size_t)4 * 160 * 16 + 4 * 8 * 64) * sizeof(double);
  static DynLdsCache g0{}, g1{};
  ensure_dyn_lds(ew_vatom_kernel<0>, lds, g0);
  ensure_dyn_lds(ew_vatom_kernel<1>, lds, g1);
  hipLaunchKernelGGL(ew_vatom_kernel<0>, dim3(nb_pad / 64, 4), dim3(512), lds, s, pl.C_pad, nb_pad, pl.n_col_tiles, kzt, ux, uy, uz,
                     ct_ptr, tiles, pl.p_ikx, pl.p_iky, pl.p_sgn, Gwf2, Rp, Tz, out);
  hipLaunchKernelGGL(ew_vatom_kernel<1>, dim3(nb_pad / 64, 4), dim3(512), lds, s, pl.C_pad, nb_pad, pl.n_col_tiles, kzt, ux, uy, uz,
                     ct_ptr, tiles, pl.p_ikx, pl.p_iky, pl.p_sgn, Gwf2, Rp, Tz, out);
}

void launch_ew_vatom_out(hipStream_t s, int n, int nb_pad, const double *bk, const double *vk, const int *idx, const double *q, double qs,
                         double *vo) {
  if (n <= 0) return;
  hipLaunchKernelGGL(ew_vatom_out_kernel<false>, dim3((n + 255) / 256), dim3(256), 0, s, n, nb_pad, bk, vk, idx, q, qs, 0, vo);
}

void launch_ew_vatom_out_device(hipStream_t s, int n, int nb_pad, const double *bk, const double *vk, const double *q, double qs, int base,
                                double *vo) {
  if (n <= 0) return;
  hipLaunchKernelGGL(ew_vatom_out_kernel<true>, dim3((n + 255) / 256), dim3(256), 0, s, n, nb_pad, bk, vk, (const int *)nullptr, q, qs,
                     base, vo);
}

int kspace_four_sums_workgroups(int n) { return std::max(1, std::min(256, (n + 255) / 256)); }

void launch_kspace_four_sums(hipStream_t s, int n, const double *x, const double *q, double *part, double *sums) {
  const int nwg = kspace_four_sums_workgroups(n);
  hipLaunchKernelGGL(kspace_four_sums_kernel, dim3(nwg), dim3(256), 0, s, n, x, q, (const double *)nullptr, 0, part, 0);
  hipLaunchKernelGGL(kspace_four_sums_kernel, dim3(1), dim3(256), 0, s, n, x, q, (const double *)part, nwg, sums, 1);
}

void launch_kspace_finish(hipStream_t s, const KspaceFinish &a, const double *s7, const double *four, double *ev) {
  hipLaunchKernelGGL(kspace_finish_kernel, dim3(1), dim3(64), 0, s, a, s7, four, ev);
}

}  // namespace conp
