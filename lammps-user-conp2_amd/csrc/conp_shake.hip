// SHAKE bond and angle constraints of `fix shake` -- the conp_shake_* entries of include/conp_hip.h, DESIGN.md section 23.
//
// The arithmetic is LAMMPS' FixShake @ 27May2021 (shake, shake3, shake3angle) without rRESPA, rmass or RATTLE, restated in the
// header.  Products are kept as written (fp contract off).  A cluster is two or three owned atoms that belong to no other cluster,
// so nothing meets an atomic and nothing goes through scratch memory:
//
//   shake_kernel<MODE>    one thread per cluster: gathers its atoms, forms the unconstrained positions in registers (there is no
//                         xshake array), solves for the multipliers, and adds the constraint force to f (SHAKE_FORCE) or moves x by
//                         it (SHAKE_CORRECT).  With d_vatom, thread i < nlocal also zeroes the row of an atom in no cluster (the
//                         rows of cluster atoms are stored by their cluster's thread).  With d_out, each workgroup -- one wave --
//                         leaves a row of partial sums: the virial through a fixed shuffle tree, two counts and the largest niter.
//   shake_check_kernel    one thread per cluster: the largest |r - d| / d of its bonds and of its 1-2 distance, per workgroup.
//   shake_finish_kernel   one workgroup: adds (or takes the maximum of) the rows in a fixed order, as integrate_finish_kernel does.
//
// Atoms in no cluster and rows from nlocal on are neither loaded nor stored.  A workgroup is one wave: there is no barrier in the
// cluster kernels, and none behind a return in the finishing one.
#include <hip/hip_runtime.h>

#include "conp_kernels.h"

namespace conp {

namespace {

struct V3 { double x, y, z; };

__device__ __forceinline__ double dot(const V3 &a, const V3 &b) {
#pragma clang fp contract(off)
  return a.x * b.x + a.y * b.y + a.z * b.z;
}

// one pass of the minimum image along a dimension with prd > 0
__device__ __forceinline__ double image(double d, double prd) {
#pragma clang fp contract(off)
  if (prd > 0.0 && fabs(d) > 0.5 * prd) {
    if (d < 0.0) d += prd;
    else d -= prd;
  }
  return d;
}

__device__ __forceinline__ V3 diff(const V3 &a, const V3 &b, const ShakeArgs &A) {
#pragma clang fp contract(off)
  V3 d;
  d.x = image(a.x - b.x, A.prd[0]);
  d.y = image(a.y - b.y, A.prd[1]);
  d.z = image(a.z - b.z, A.prd[2]);
  return d;
}

__device__ __forceinline__ V3 load3(const double *p, size_t o) {
  V3 r;
  r.x = p[o]; r.y = p[o + 1]; r.z = p[o + 2];
  return r;
}

struct Atom {
  size_t o;              // 3 i
  double im, dtfmsq;
  V3 x, xs, f;           // f: the row as loaded (SHAKE_FORCE) or 0.0 (SHAKE_CORRECT)
};

template <int MODE>
__device__ __forceinline__ Atom load_atom(const ShakeArgs &a, int i) {
#pragma clang fp contract(off)
  Atom t;
  t.o = 3 * (size_t)i;
  const double m = a.mass[a.type[i]];
  t.im = 1.0 / m;
  t.dtfmsq = a.dtfsq / m;
  t.x = load3(a.x, t.o);
  if (MODE == SHAKE_FORCE) {
    const V3 v = load3(a.v, t.o);
    t.f = load3(a.f, t.o);
    t.xs.x = t.x.x + a.dtv * v.x + t.dtfmsq * t.f.x;
    t.xs.y = t.x.y + a.dtv * v.y + t.dtfmsq * t.f.y;
    t.xs.z = t.x.z + a.dtv * v.z + t.dtfmsq * t.f.z;
  } else {
    t.f.x = 0.0; t.f.y = 0.0; t.f.z = 0.0;
    t.xs = t.x;
  }
  return t;
}

// f (SHAKE_FORCE) or x += dtfmsq f (SHAKE_CORRECT) of one cluster atom
template <int MODE>
__device__ __forceinline__ void store_atom(const ShakeArgs &a, const Atom &t) {
#pragma clang fp contract(off)
  if (MODE == SHAKE_FORCE) {
    a.f[t.o] = t.f.x; a.f[t.o + 1] = t.f.y; a.f[t.o + 2] = t.f.z;
  } else {
    a.x[t.o] = t.x.x + t.dtfmsq * t.f.x;
    a.x[t.o + 1] = t.x.y + t.dtfmsq * t.f.y;
    a.x[t.o + 2] = t.x.z + t.dtfmsq * t.f.z;
  }
}

__device__ __forceinline__ void store_vatom(double *vatom, size_t o3, const double (&v)[6], double n) {
  double *row = vatom + 2 * o3;
#pragma unroll
  for (int k = 0; k < 6; ++k) row[k] = v[k] / n;
}

__device__ __forceinline__ double shake_wave_sum(double v) {
#pragma clang fp contract(off)
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
  return v;
}

__device__ __forceinline__ double shake_wave_max(double v) {
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) v = fmax(v, __shfl_down(v, off, 64));
  return v;
}

template <int MODE>
__global__ __launch_bounds__(SHAKE_BLOCK) void shake_kernel(ShakeArgs a) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * SHAKE_BLOCK + threadIdx.x;
  double v[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  double unconverged = 0.0, bad_determ = 0.0, iterations = 0.0;
  if (k < a.ncluster) {
    const int *c = a.cluster + 7 * (size_t)k;
    const int flag = c[0];
    const double tol = a.tolerance;
    if (flag == 2) {
      Atom p0 = load_atom<MODE>(a, c[1]), p1 = load_atom<MODE>(a, c[2]);
      const double d0 = a.bond_d[c[4]];
      const V3 r01 = diff(p0.x, p1.x, a), s01 = diff(p0.xs, p1.xs, a);
      const double r01sq = dot(r01, r01), s01sq = dot(s01, s01);
      const double qa = (p0.im + p1.im) * (p0.im + p1.im) * r01sq;
      const double qb = 2.0 * (p0.im + p1.im) * dot(s01, r01);
      const double qc = s01sq - d0 * d0;
      double determ = qb * qb - 4.0 * qa * qc;
      if (determ < 0.0) { determ = 0.0; bad_determ = 1.0; }
      double lamda;
      if (qb > 0.0) lamda = (-qb + sqrt(determ)) / (2.0 * qa);
      else lamda = (-qb - sqrt(determ)) / (2.0 * qa);
      lamda /= a.dtfsq;
      p0.f.x += lamda * r01.x; p0.f.y += lamda * r01.y; p0.f.z += lamda * r01.z;
      p1.f.x -= lamda * r01.x; p1.f.y -= lamda * r01.y; p1.f.z -= lamda * r01.z;
      store_atom<MODE>(a, p0); store_atom<MODE>(a, p1);
      v[0] = lamda * r01.x * r01.x; v[1] = lamda * r01.y * r01.y; v[2] = lamda * r01.z * r01.z;
      v[3] = lamda * r01.x * r01.y; v[4] = lamda * r01.x * r01.z; v[5] = lamda * r01.y * r01.z;
      if (MODE == SHAKE_FORCE && a.vatom) { store_vatom(a.vatom, p0.o, v, 2.0); store_vatom(a.vatom, p1.o, v, 2.0); }
    } else {
      Atom p0 = load_atom<MODE>(a, c[1]), p1 = load_atom<MODE>(a, c[2]), p2 = load_atom<MODE>(a, c[3]);
      const double d0 = a.bond_d[c[4]], d1 = a.bond_d[c[5]];
      const V3 r01 = diff(p0.x, p1.x, a), r02 = diff(p0.x, p2.x, a);
      const V3 s01 = diff(p0.xs, p1.xs, a), s02 = diff(p0.xs, p2.xs, a);
      const double r01sq = dot(r01, r01), r02sq = dot(r02, r02), s01sq = dot(s01, s01), s02sq = dot(s02, s02);
      const double im0 = p0.im, im1 = p1.im, im2 = p2.im;
      const double r0102 = dot(r01, r02);
      double l01 = 0.0, l02 = 0.0, l12 = 0.0;
      V3 r12;
      r12.x = 0.0; r12.y = 0.0; r12.z = 0.0;
      bool done = false, solved = true;
      int niter = 0;
      if (flag == 3) {
        const double a11 = 2.0 * (im0 + im1) * dot(s01, r01);
        const double a12 = 2.0 * im0 * dot(s01, r02);
        const double a21 = 2.0 * im0 * dot(s02, r01);
        const double a22 = 2.0 * (im0 + im2) * dot(s02, r02);
        const double determ = a11 * a22 - a12 * a21;
        if (determ == 0.0) {
          solved = false;
        } else {
          const double determinv = 1.0 / determ;
          const double a11inv = a22 * determinv, a12inv = -a12 * determinv, a21inv = -a21 * determinv, a22inv = a11 * determinv;
          const double q1_0101 = (im0 + im1) * (im0 + im1) * r01sq, q1_0202 = im0 * im0 * r02sq, q1_0102 = 2.0 * (im0 + im1) * im0 * r0102;
          const double q2_0202 = (im0 + im2) * (im0 + im2) * r02sq, q2_0101 = im0 * im0 * r01sq, q2_0102 = 2.0 * (im0 + im2) * im0 * r0102;
          while (!done && niter < a.max_iter) {
            const double quad1 = q1_0101 * l01 * l01 + q1_0202 * l02 * l02 + q1_0102 * l01 * l02;
            const double quad2 = q2_0101 * l01 * l01 + q2_0202 * l02 * l02 + q2_0102 * l01 * l02;
            const double b1 = d0 * d0 - s01sq - quad1;
            const double b2 = d1 * d1 - s02sq - quad2;
            const double n01 = a11inv * b1 + a12inv * b2;
            const double n02 = a21inv * b1 + a22inv * b2;
            done = true;
            if (fabs(n01 - l01) > tol) done = false;
            if (fabs(n02 - l02) > tol) done = false;
            l01 = n01; l02 = n02;
            if (fabs(l01) > 1e150 || fabs(l02) > 1e150) done = true;
            niter++;
          }
        }
      } else {
        const double d2 = a.angle_d[c[6]];
        r12 = diff(p1.x, p2.x, a);
        const V3 s12 = diff(p1.xs, p2.xs, a);
        const double r12sq = dot(r12, r12), s12sq = dot(s12, s12);
        const double r0112 = dot(r01, r12), r0212 = dot(r02, r12);
        const double a11 = 2.0 * (im0 + im1) * dot(s01, r01);
        const double a12 = 2.0 * im0 * dot(s01, r02);
        const double a13 = -2.0 * im1 * dot(s01, r12);
        const double a21 = 2.0 * im0 * dot(s02, r01);
        const double a22 = 2.0 * (im0 + im2) * dot(s02, r02);
        const double a23 = 2.0 * im2 * dot(s02, r12);
        const double a31 = -2.0 * im1 * dot(s12, r01);
        const double a32 = 2.0 * im2 * dot(s12, r02);
        const double a33 = 2.0 * (im1 + im2) * dot(s12, r12);
        const double determ = a11 * a22 * a33 + a12 * a23 * a31 + a13 * a21 * a32 - a11 * a23 * a32 - a12 * a21 * a33 - a13 * a22 * a31;
        if (determ == 0.0) {
          solved = false;
        } else {
          const double determinv = 1.0 / determ;
          const double a11inv = determinv * (a22 * a33 - a23 * a32);
          const double a12inv = -determinv * (a12 * a33 - a13 * a32);
          const double a13inv = determinv * (a12 * a23 - a13 * a22);
          const double a21inv = -determinv * (a21 * a33 - a23 * a31);
          const double a22inv = determinv * (a11 * a33 - a13 * a31);
          const double a23inv = -determinv * (a11 * a23 - a13 * a21);
          const double a31inv = determinv * (a21 * a32 - a22 * a31);
          const double a32inv = -determinv * (a11 * a32 - a12 * a31);
          const double a33inv = determinv * (a11 * a22 - a12 * a21);
          const double q1_0101 = (im0 + im1) * (im0 + im1) * r01sq, q1_0202 = im0 * im0 * r02sq, q1_1212 = im1 * im1 * r12sq;
          const double q1_0102 = 2.0 * (im0 + im1) * im0 * r0102, q1_0112 = -2.0 * (im0 + im1) * im1 * r0112, q1_0212 = -2.0 * im0 * im1 * r0212;
          const double q2_0101 = im0 * im0 * r01sq, q2_0202 = (im0 + im2) * (im0 + im2) * r02sq, q2_1212 = im2 * im2 * r12sq;
          const double q2_0102 = 2.0 * (im0 + im2) * im0 * r0102, q2_0112 = 2.0 * im0 * im2 * r0112, q2_0212 = 2.0 * (im0 + im2) * im2 * r0212;
          const double q3_0101 = im1 * im1 * r01sq, q3_0202 = im2 * im2 * r02sq, q3_1212 = (im1 + im2) * (im1 + im2) * r12sq;
          const double q3_0102 = -2.0 * im1 * im2 * r0102, q3_0112 = -2.0 * (im1 + im2) * im1 * r0112, q3_0212 = 2.0 * (im1 + im2) * im2 * r0212;
          while (!done && niter < a.max_iter) {
            const double quad1 = q1_0101 * l01 * l01 + q1_0202 * l02 * l02 + q1_1212 * l12 * l12 + q1_0102 * l01 * l02 + q1_0112 * l01 * l12 + q1_0212 * l02 * l12;
            const double quad2 = q2_0101 * l01 * l01 + q2_0202 * l02 * l02 + q2_1212 * l12 * l12 + q2_0102 * l01 * l02 + q2_0112 * l01 * l12 + q2_0212 * l02 * l12;
            const double quad3 = q3_0101 * l01 * l01 + q3_0202 * l02 * l02 + q3_1212 * l12 * l12 + q3_0102 * l01 * l02 + q3_0112 * l01 * l12 + q3_0212 * l02 * l12;
            const double b1 = d0 * d0 - s01sq - quad1;
            const double b2 = d1 * d1 - s02sq - quad2;
            const double b3 = d2 * d2 - s12sq - quad3;
            const double n01 = a11inv * b1 + a12inv * b2 + a13inv * b3;
            const double n02 = a21inv * b1 + a22inv * b2 + a23inv * b3;
            const double n12 = a31inv * b1 + a32inv * b2 + a33inv * b3;
            done = true;
            if (fabs(n01 - l01) > tol) done = false;
            if (fabs(n02 - l02) > tol) done = false;
            if (fabs(n12 - l12) > tol) done = false;
            l01 = n01; l02 = n02; l12 = n12;
            if (fabs(l01) > 1e150 || fabs(l02) > 1e150 || fabs(l12) > 1e150) done = true;
            niter++;
          }
        }
      }
      if (!solved) {
        bad_determ = 1.0;                       // the cluster adds nothing: f and x stay as they are
      } else {
        if (!done) unconverged = 1.0;
        iterations = (double)niter;
        l01 /= a.dtfsq; l02 /= a.dtfsq;
        p0.f.x += l01 * r01.x + l02 * r02.x; p0.f.y += l01 * r01.y + l02 * r02.y; p0.f.z += l01 * r01.z + l02 * r02.z;
        if (flag == 3) {
          p1.f.x -= l01 * r01.x; p1.f.y -= l01 * r01.y; p1.f.z -= l01 * r01.z;
          p2.f.x -= l02 * r02.x; p2.f.y -= l02 * r02.y; p2.f.z -= l02 * r02.z;
          v[0] = l01 * r01.x * r01.x + l02 * r02.x * r02.x;
          v[1] = l01 * r01.y * r01.y + l02 * r02.y * r02.y;
          v[2] = l01 * r01.z * r01.z + l02 * r02.z * r02.z;
          v[3] = l01 * r01.x * r01.y + l02 * r02.x * r02.y;
          v[4] = l01 * r01.x * r01.z + l02 * r02.x * r02.z;
          v[5] = l01 * r01.y * r01.z + l02 * r02.y * r02.z;
        } else {
          l12 /= a.dtfsq;
          p1.f.x -= l01 * r01.x - l12 * r12.x; p1.f.y -= l01 * r01.y - l12 * r12.y; p1.f.z -= l01 * r01.z - l12 * r12.z;
          p2.f.x -= l02 * r02.x + l12 * r12.x; p2.f.y -= l02 * r02.y + l12 * r12.y; p2.f.z -= l02 * r02.z + l12 * r12.z;
          v[0] = l01 * r01.x * r01.x + l02 * r02.x * r02.x + l12 * r12.x * r12.x;
          v[1] = l01 * r01.y * r01.y + l02 * r02.y * r02.y + l12 * r12.y * r12.y;
          v[2] = l01 * r01.z * r01.z + l02 * r02.z * r02.z + l12 * r12.z * r12.z;
          v[3] = l01 * r01.x * r01.y + l02 * r02.x * r02.y + l12 * r12.x * r12.y;
          v[4] = l01 * r01.x * r01.z + l02 * r02.x * r02.z + l12 * r12.x * r12.z;
          v[5] = l01 * r01.y * r01.z + l02 * r02.y * r02.z + l12 * r12.y * r12.z;
        }
        store_atom<MODE>(a, p0); store_atom<MODE>(a, p1); store_atom<MODE>(a, p2);
      }
      if (MODE == SHAKE_FORCE && a.vatom) {
        store_vatom(a.vatom, p0.o, v, 3.0); store_vatom(a.vatom, p1.o, v, 3.0); store_vatom(a.vatom, p2.o, v, 3.0);
      }
    }
  }
  if (MODE == SHAKE_FORCE) {
    if (a.vatom && k < a.nlocal && !a.member[k]) {
      double *row = a.vatom + 6 * (size_t)k;
#pragma unroll
      for (int j = 0; j < 6; ++j) row[j] = 0.0;
    }
    if (a.part) {
#pragma unroll
      for (int j = 0; j < 6; ++j) v[j] = shake_wave_sum(v[j]);
      unconverged = shake_wave_sum(unconverged);
      bad_determ = shake_wave_sum(bad_determ);
      iterations = shake_wave_max(iterations);
      if (threadIdx.x == 0) {
        double *row = a.part + SHAKE_PART_W * (size_t)blockIdx.x;
#pragma unroll
        for (int j = 0; j < 6; ++j) row[j] = v[j];
        row[6] = unconverged; row[7] = bad_determ; row[8] = iterations;
      }
    }
  }
}

__global__ __launch_bounds__(SHAKE_BLOCK) void shake_check_kernel(ShakeArgs a) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * SHAKE_BLOCK + threadIdx.x;
  double bond = 0.0, angle = 0.0;
  if (k < a.ncluster) {
    const int *c = a.cluster + 7 * (size_t)k;
    const int flag = c[0];
    const V3 x0 = load3(a.x, 3 * (size_t)c[1]), x1 = load3(a.x, 3 * (size_t)c[2]);
    const V3 r01 = diff(x0, x1, a);
    const double d0 = a.bond_d[c[4]];
    bond = fabs(sqrt(dot(r01, r01)) - d0) / d0;
    if (flag != 2) {
      const V3 x2 = load3(a.x, 3 * (size_t)c[3]);
      const V3 r02 = diff(x0, x2, a);
      const double d1 = a.bond_d[c[5]];
      bond = fmax(bond, fabs(sqrt(dot(r02, r02)) - d1) / d1);
      if (flag == 1) {
        const V3 r12 = diff(x1, x2, a);
        const double d2 = a.angle_d[c[6]];
        angle = fabs(sqrt(dot(r12, r12)) - d2) / d2;
      }
    }
  }
  bond = shake_wave_max(bond);
  angle = shake_wave_max(angle);
  if (threadIdx.x == 0) {
    double *row = a.part + SHAKE_PART_W * (size_t)blockIdx.x;
    row[0] = bond; row[1] = angle;
  }
}

// out[k], k < ncol: over the rows, the sum (k < nsum) or the maximum of column k
__global__ __launch_bounds__(SHAKE_FINISH) void shake_finish_kernel(const double *part, int nrows, int nsum, int ncol, double *out) {
#pragma clang fp contract(off)
  __shared__ double red[SHAKE_FINISH / 64][SHAKE_PART_W];
  double s[SHAKE_PART_W];
#pragma unroll
  for (int k = 0; k < SHAKE_PART_W; ++k) s[k] = 0.0;
  for (int r = threadIdx.x; r < nrows; r += SHAKE_FINISH) {
#pragma unroll
    for (int k = 0; k < SHAKE_PART_W; ++k)
      if (k < ncol) {
        const double t = part[SHAKE_PART_W * (size_t)r + k];
        s[k] = k < nsum ? s[k] + t : fmax(s[k], t);
      }
  }
#pragma unroll
  for (int k = 0; k < SHAKE_PART_W; ++k) s[k] = k < nsum ? shake_wave_sum(s[k]) : shake_wave_max(s[k]);
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int k = 0; k < SHAKE_PART_W; ++k) red[threadIdx.x >> 6][k] = s[k];
  }
  __syncthreads();
  if (threadIdx.x < ncol) {
    const int k = threadIdx.x;
    double t = 0.0;
    for (int w = 0; w < SHAKE_FINISH / 64; ++w) t = k < nsum ? t + red[w][k] : fmax(t, red[w][k]);
    out[k] = t;
  }
}

}  // namespace

void launch_shake(hipStream_t s, const ShakeArgs &a, int mode, double *out) {
  const int nrows = shake_rows(a.vatom && a.nlocal > a.ncluster ? a.nlocal : a.ncluster);
  if (mode == SHAKE_CORRECT) hipLaunchKernelGGL((shake_kernel<SHAKE_CORRECT>), dim3(nrows), dim3(SHAKE_BLOCK), 0, s, a);
  else hipLaunchKernelGGL((shake_kernel<SHAKE_FORCE>), dim3(nrows), dim3(SHAKE_BLOCK), 0, s, a);
  if (out) hipLaunchKernelGGL(shake_finish_kernel, dim3(1), dim3(SHAKE_FINISH), 0, s, a.part, nrows, 8, SHAKE_PART_W, out);
}

void launch_shake_check(hipStream_t s, const ShakeArgs &a, double *out) {
  const int nrows = shake_rows(a.ncluster);
  hipLaunchKernelGGL(shake_check_kernel, dim3(nrows), dim3(SHAKE_BLOCK), 0, s, a);
  hipLaunchKernelGGL(shake_finish_kernel, dim3(1), dim3(SHAKE_FINISH), 0, s, a.part, nrows, 0, 2, out);
}

}  // namespace conp
