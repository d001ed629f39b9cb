// Torsional forces of `dihedral_style opls | harmonic` and `improper_style harmonic | cvff` -- conp_dihedral_compute /
// conp_dihedral_compute_device of include/conp_hip.h, DESIGN.md section 28.
//
// The arithmetic is the header's, one geometry for all four styles: phi by atan2 and its gradient without 1 / sin(phi).  Products are
// kept as written (fp contract off).  No output meets an atomic -- the three-kernel scheme of conp_bonded.hip:
//
//   dihedral_term_kernel    <EV>: one thread per term, dihedrals first, then impropers.  Writes the term's record (DIHEDRAL_TERM_W
//                           doubles, 128 aligned bytes as eight 16-byte stores: the force on member 1, on 3, on 4, the energy, the
//                           six virial products) into scratch.  EV: the term's weighted tallies (edihedral, eimproper, virial[6])
//                           are reduced over the workgroup in a fixed tree and stored as one row per workgroup.
//   dihedral_finish_kernel  adds the rows in a fixed order, nothing cleared, one workgroup.
//   dihedral_gather_kernel  one thread per atom: walks the atom's (term, role) slots in the order conp_dihedral_set_lists stored
//                           them, sums the records' shares from 0.0 and adds the force to f once; eatom / vatom are written for
//                           every row (0.0 for an atom in no term), f is touched only for atoms with slots.
#include <hip/hip_runtime.h>

#include "conp_kernels.h"

namespace conp {

namespace {

enum { FORM_OPLS, FORM_COSINE, FORM_QUADRATIC };         // the three energy functions of the four styles

__device__ __forceinline__ double dihedral_wave_sum(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

// x_b seen from x_a: the closest image along a dimension of length prd (0: as it is); the product first, then the sum
__device__ __forceinline__ double dihedral_image(double xa, double xb, double prd) {
#pragma clang fp contract(off)
  if (!(prd > 0.0)) return xb;
  const double d = xa - xb, h = prd / 2;
  const int s = d > h ? 1 : (d < -h ? -1 : 0);
  const double shift = (double)s * prd;
  return xb + shift;
}

template <bool EV>
__global__ __launch_bounds__(DIHEDRAL_BLOCK) void dihedral_term_kernel(DihedralArgs a) {
#pragma clang fp contract(off)
  __shared__ double red[DIHEDRAL_BLOCK / 64][8];
  const int nterm = a.ndihedral + a.nimproper;
  const int t = blockIdx.x * DIHEDRAL_BLOCK + threadIdx.x;
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (t < nterm) {
    const bool imp = t >= a.ndihedral;
    const int *m = imp ? a.improper + 5 * (size_t)(t - a.ndihedral) : a.dihedral + 5 * (size_t)t;
    const int i1 = m[0], i2 = m[1], i3 = m[2], i4 = m[3], ty = m[4];
    const double *x1 = a.x + 3 * (size_t)i1, *x2 = a.x + 3 * (size_t)i2, *x3 = a.x + 3 * (size_t)i3, *x4 = a.x + 3 * (size_t)i4;
    double F[3], G[3], H[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double p2 = x2[c];
      const double p3 = dihedral_image(p2, x3[c], a.prd[c]);
      F[c] = dihedral_image(p2, x1[c], a.prd[c]) - p2;
      G[c] = p2 - p3;
      H[c] = dihedral_image(p3, x4[c], a.prd[c]) - p3;
    }
    const double Ax = F[1] * G[2] - F[2] * G[1], Ay = F[2] * G[0] - F[0] * G[2], Az = F[0] * G[1] - F[1] * G[0];
    const double Bx = H[1] * G[2] - H[2] * G[1], By = H[2] * G[0] - H[0] * G[2], Bz = H[0] * G[1] - H[1] * G[0];
    const double A2 = Ax * Ax + Ay * Ay + Az * Az, B2 = Bx * Bx + By * By + Bz * Bz;
    const double g = sqrt(G[0] * G[0] + G[1] * G[1] + G[2] * G[2]);
    double f1[3] = {0.0, 0.0, 0.0}, f3[3] = {0.0, 0.0, 0.0}, f4[3] = {0.0, 0.0, 0.0}, e = 0.0;
    double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (A2 != 0.0 && B2 != 0.0 && g != 0.0) {
      const double Cx = By * Az - Bz * Ay, Cy = Bz * Ax - Bx * Az, Cz = Bx * Ay - By * Ax;
      const double y = (Cx * G[0] + Cy * G[1] + Cz * G[2]) / g;
      const double phi = atan2(y, Ax * Bx + Ay * By + Az * Bz);
      const int form = imp ? (a.istyle == IMPROPER_CVFF ? FORM_COSINE : FORM_QUADRATIC) : (a.dstyle == DIHEDRAL_OPLS ? FORM_OPLS : FORM_COSINE);
      const double *k = (imp ? a.icoef : a.dcoef) + 4 * (size_t)ty;
      double de;
      if (form == FORM_OPLS) {
        const double p2 = 2.0 * phi, p3 = 3.0 * phi, p4 = 4.0 * phi;
        const double s1 = sin(phi), c1 = cos(phi), s2 = sin(p2), c2 = cos(p2), s3 = sin(p3), c3 = cos(p3), s4 = sin(p4), c4 = cos(p4);
        e = 0.5 * (k[0] * (1.0 + c1) + k[1] * (1.0 - c2) + k[2] * (1.0 + c3) + k[3] * (1.0 - c4));
        de = 0.5 * (2.0 * (k[1] * s2) - k[0] * s1 - 3.0 * (k[2] * s3) + 4.0 * (k[3] * s4));
      } else if (form == FORM_COSINE) {                  // dihedral harmonic and improper cvff: K d n
        const double an = k[2] * phi;
        e = k[0] * (1.0 + k[1] * cos(an));
        de = -(k[0] * k[1] * k[2] * sin(an));
      } else {                                           // improper harmonic: K chi0
        const double u = fabs(phi) - k[1];
        e = k[0] * u * u;
        de = 2.0 * k[0] * (phi - copysign(k[1], phi));
      }
      const double p = -de;
      const double ga = g / A2, gb = g / B2;
      const double sa = (F[0] * G[0] + F[1] * G[1] + F[2] * G[2]) / (A2 * g), sb = (H[0] * G[0] + H[1] * G[1] + H[2] * G[2]) / (B2 * g);
      const double Av[3] = {Ax, Ay, Az}, Bv[3] = {Bx, By, Bz};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double d1 = -(ga * Av[c]), d4 = gb * Bv[c], sc = sa * Av[c] - sb * Bv[c];
        const double d3 = (-d4) - sc;
        f1[c] = p * d1; f3[c] = p * d3; f4[c] = p * d4;
      }
      const double u3[3] = {-G[0], -G[1], -G[2]}, u4[3] = {H[0] - G[0], H[1] - G[1], H[2] - G[2]};
      v[0] = F[0] * f1[0] + u3[0] * f3[0] + u4[0] * f4[0];
      v[1] = F[1] * f1[1] + u3[1] * f3[1] + u4[1] * f4[1];
      v[2] = F[2] * f1[2] + u3[2] * f3[2] + u4[2] * f4[2];
      v[3] = F[0] * f1[1] + u3[0] * f3[1] + u4[0] * f4[1];
      v[4] = F[0] * f1[2] + u3[0] * f3[2] + u4[0] * f4[2];
      v[5] = F[1] * f1[2] + u3[1] * f3[2] + u4[1] * f4[2];
    }
    // the record: 128 bytes at a 128-byte boundary, 16 bytes per store
    double2 *rec = reinterpret_cast<double2 *>(a.term + (size_t)t * DIHEDRAL_TERM_W);
    rec[0] = make_double2(f1[0], f1[1]); rec[1] = make_double2(f1[2], f3[0]);
    rec[2] = make_double2(f3[1], f3[2]); rec[3] = make_double2(f4[0], f4[1]);
    rec[4] = make_double2(f4[2], e);     rec[5] = make_double2(v[0], v[1]);
    rec[6] = make_double2(v[2], v[3]);   rec[7] = make_double2(v[4], v[5]);
    if (EV) {
      const int slot = imp ? 1 : 0;
      if (a.newton) {
        s[slot] = e;
#pragma unroll
        for (int k = 0; k < 6; ++k) s[2 + k] = v[k];
      } else {
        const bool o1 = i1 < a.nlocal, o2 = i2 < a.nlocal, o3 = i3 < a.nlocal, o4 = i4 < a.nlocal;
        const double eq = 0.25 * e;
        double es = 0.0;
        if (o1) es += eq;
        if (o2) es += eq;
        if (o3) es += eq;
        if (o4) es += eq;
        s[slot] = es;
#pragma unroll
        for (int k = 0; k < 6; ++k) {
          const double vq = 0.25 * v[k];
          if (o1) s[2 + k] += vq;
          if (o2) s[2 + k] += vq;
          if (o3) s[2 + k] += vq;
          if (o4) s[2 + k] += vq;
        }
      }
    }
  }
  if (!EV) return;
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = dihedral_wave_sum(s[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) red[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    double tsum = 0.0;
    for (int w = 0; w < DIHEDRAL_BLOCK / 64; ++w) tsum += red[w][threadIdx.x];
    a.part[8 * (size_t)blockIdx.x + threadIdx.x] = tsum;
  }
}

// ev[k] = sum over the rows of part[row][k], k < 8: every thread adds its rows in ascending order, then one fixed tree
__global__ __launch_bounds__(DIHEDRAL_FINISH) void dihedral_finish_kernel(int nrows, const double *__restrict__ part, double *__restrict__ ev) {
#pragma clang fp contract(off)
  __shared__ double red[DIHEDRAL_FINISH / 64][8];
  double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int r = threadIdx.x; r < nrows; r += DIHEDRAL_FINISH) {
#pragma unroll
    for (int k = 0; k < 8; ++k) s[k] += part[8 * (size_t)r + k];
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) s[k] = dihedral_wave_sum(s[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k) red[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < 8) {
    double t = 0.0;
    for (int w = 0; w < DIHEDRAL_FINISH / 64; ++w) t += red[w][threadIdx.x];
    ev[threadIdx.x] = t;
  }
}

__global__ __launch_bounds__(DIHEDRAL_BLOCK) void dihedral_gather_kernel(DihedralArgs a) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * DIHEDRAL_BLOCK + threadIdx.x;
  if (i >= a.nall) return;
  const bool active = a.newton || i < a.nlocal;
  const int b = a.slot_ptr[i], e = active ? a.slot_ptr[i + 1] : b;
  double fx = 0.0, fy = 0.0, fz = 0.0, ei = 0.0;
  double vi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int k = b; k < e; ++k) {
    const int sl = a.slot[k], t = sl >> 2, role = sl & 3;
    const double *rec = a.term + (size_t)t * DIHEDRAL_TERM_W;
    if (role == 0) { fx += rec[0]; fy += rec[1]; fz += rec[2]; }
    else if (role == 2) { fx += rec[3]; fy += rec[4]; fz += rec[5]; }
    else if (role == 3) { fx += rec[6]; fy += rec[7]; fz += rec[8]; }
    else { fx -= (rec[0] + rec[3]) + rec[6]; fy -= (rec[1] + rec[4]) + rec[7]; fz -= (rec[2] + rec[5]) + rec[8]; }
    if (a.eatom) ei += rec[9] * 0.25;
    if (a.vatom) {
#pragma unroll
      for (int c = 0; c < 6; ++c) vi[c] += rec[10 + c] * 0.25;
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

void launch_dihedral(hipStream_t s, const DihedralArgs &a, double *ev) {
  const int nterm = a.ndihedral + a.nimproper, nrows = (nterm + DIHEDRAL_BLOCK - 1) / DIHEDRAL_BLOCK;
  if (nterm > 0) {
    if (ev) hipLaunchKernelGGL((dihedral_term_kernel<true>), dim3(nrows), dim3(DIHEDRAL_BLOCK), 0, s, a);
    else hipLaunchKernelGGL((dihedral_term_kernel<false>), dim3(nrows), dim3(DIHEDRAL_BLOCK), 0, s, a);
  }
  if (ev) hipLaunchKernelGGL(dihedral_finish_kernel, dim3(1), dim3(DIHEDRAL_FINISH), 0, s, nrows, a.part, ev);
  if ((a.f || a.eatom || a.vatom) && a.nall > 0)
    hipLaunchKernelGGL(dihedral_gather_kernel, dim3((a.nall + DIHEDRAL_BLOCK - 1) / DIHEDRAL_BLOCK), dim3(DIHEDRAL_BLOCK), 0, s, a);
}

}  // namespace conp
