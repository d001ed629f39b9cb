// Ghost atoms of one rank in a periodic box, on the device -- conp_ghost_build_device / conp_ghost_fill_device /
// conp_ghost_fill_int_device / conp_ghost_fold_device / conp_atoms_wrap_device of include/conp_hip.h, DESIGN.md section 18: LAMMPS'
// Comm::borders, forward_comm and reverse_comm, and the remap into the box that precedes a ghost build.  The map is the one
// conp_amd/neighbor.py::make_ghosts defines; nothing in it depends on which thread arrives first.
//
//   ghost_image_kernel    <FILL>: one wavefront per block of 64 owners, four per workgroup.  The shifts are walked in their order
//                         (sx slowest, sz fastest); each lane tests its owner's image, kept images are ranked with a ballot and a
//                         popcount prefix.  The count pass writes count[shift][block] and the images per owner; the fill pass --
//                         the same code, behind the two exclusive scans (neigh_scan_kernel) -- writes owner and img of ghost
//                         start[shift][block] + rank, and that ghost index into the owner's list, which therefore ascends
//   ghost_fill_xq_kernel  x of every ghost = x_owner + img * prd, q = q_owner when a charge array is given
//   ghost_fill_int_kernel `width` ints per ghost copied from the owner's row
//   ghost_fold_kernel     one thread per owner and component: v[o] = ((v[o] + v[g1]) + v[g2]) + .. over the owner's list
//   atoms_wrap_kernel     owned atoms remapped into the box, one pass per periodic dimension, with optional image counters
#include <hip/hip_runtime.h>

#include "conp_kernels.h"

namespace conp {

namespace {

template <bool FILL>
__global__ __launch_bounds__(256) void ghost_image_kernel(GhostBuildArgs a) {
#pragma clang fp contract(off)
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= a.nblock) return;                     // (whole waves leave; the kernel has no barrier)
  const int o = w * 64 + lane;
  const bool valid = o < a.nlocal;
  double x[3] = {0.0, 0.0, 0.0};
  if (valid) {
#pragma unroll
    for (int c = 0; c < 3; ++c) x[c] = a.x[3 * (size_t)o + c];
  }
  const unsigned long long below = (1ull << lane) - 1ull;
  const int ofirst = FILL && valid ? a.ofirst[o] : 0;
  const int room = FILL && valid ? a.nimg[o] : 0;     // what the count pass found: the fill pass never stores past it
  int k = 0;
  for (int s = 0; s < a.nshift; ++s) {                // the trip count is the same for every lane: the ballot sees the whole wave
    bool keep = valid;
    int sh[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      sh[c] = a.shift[3 * s + c];
      const double d = (double)sh[c] * a.prd[c];      // the product first, then the sum: Comm::pack_comm, ghost_fill_kernel
      const double xi = x[c] + d;
      keep = keep && xi >= a.lo[c] && xi < a.hi[c];   // (a NaN or infinite coordinate fails)
    }
    const unsigned long long vote = __ballot(keep);
    const size_t e = (size_t)s * a.nblock + w;
    if (!FILL) {
      if (lane == 0) a.count[e] = __popcll(vote);
    } else if (keep) {
      const int g = a.start[e] + __popcll(vote & below);
      if (g < a.nghost && k < room) {
        a.owner[g] = o;
        a.img[3 * (size_t)g] = sh[0]; a.img[3 * (size_t)g + 1] = sh[1]; a.img[3 * (size_t)g + 2] = sh[2];
        a.list[ofirst + k] = g;
      }
    }
    k += keep;
  }
  if (!FILL && valid) a.nimg[o] = k;
}

// ghost_fill_kernel of conp_kernels.hip (the host-array path) with an optional charge array and 64-bit row offsets
__global__ __launch_bounds__(256) void ghost_fill_xq_kernel(int nlocal, int nghost, const int *__restrict__ owner, const int *__restrict__ img,
                                                            double px, double py, double pz, double *__restrict__ x, double *__restrict__ q) {
#pragma clang fp contract(off)
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= nghost) return;
  const size_t o = (size_t)owner[g], i = (size_t)nlocal + g;
  const double dx = img[3 * (size_t)g] * px, dy = img[3 * (size_t)g + 1] * py, dz = img[3 * (size_t)g + 2] * pz;
  x[3 * i] = x[3 * o] + dx; x[3 * i + 1] = x[3 * o + 1] + dy; x[3 * i + 2] = x[3 * o + 2] + dz;
  if (q) q[i] = q[o];
}

__global__ __launch_bounds__(256) void ghost_fill_int_kernel(int nlocal, long long n /*nghost * width*/, int width, const int *__restrict__ owner,
                                                             int *__restrict__ v) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= n) return;
  const long long g = t / width;
  const int c = (int)(t - g * width);
  v[((size_t)nlocal + g) * width + c] = v[(size_t)owner[g] * width + c];
}

__global__ __launch_bounds__(256) void ghost_fold_kernel(int nlocal, int width, const int *__restrict__ ofirst, const int *__restrict__ nimg,
                                                         const int *__restrict__ list, double *__restrict__ v) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= (long long)nlocal * width) return;
  const int o = (int)(t / width), c = (int)(t - (long long)o * width);
  const int b = ofirst[o], e = b + nimg[o];
  double acc = v[(size_t)o * width + c];
  for (int k = b; k < e; ++k) acc += v[((size_t)nlocal + list[k]) * width + c];
  v[(size_t)o * width + c] = acc;
}

__global__ __launch_bounds__(256) void atoms_wrap_kernel(AtomsWrapArgs a, double *__restrict__ x, int *__restrict__ image) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.nlocal) return;
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    if (!a.periodic[c]) continue;
    double v = x[3 * (size_t)i + c];
    int d = 0;
    if (v < a.lo[c]) { v += a.prd[c]; d -= 1; }
    if (v >= a.hi[c]) {
      v -= a.prd[c];
      if (v < a.lo[c]) v = a.lo[c];
      d += 1;
    }
    x[3 * (size_t)i + c] = v;
    if (image && d != 0) image[3 * (size_t)i + c] += d;
  }
}

}  // namespace

void launch_ghost_images(hipStream_t s, const GhostBuildArgs &a, bool fill) {
  if (a.nblock <= 0 || a.nshift <= 0) return;
  const dim3 grid((a.nblock + 3) / 4), block(256);
  if (fill) hipLaunchKernelGGL(ghost_image_kernel<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(ghost_image_kernel<false>, grid, block, 0, s, a);
}

void launch_ghost_fill_xq(hipStream_t s, int nlocal, int nghost, const int *owner, const int *img, double px, double py, double pz, double *x,
                          double *q) {
  if (nghost <= 0) return;
  hipLaunchKernelGGL(ghost_fill_xq_kernel, dim3((nghost + 255) / 256), dim3(256), 0, s, nlocal, nghost, owner, img, px, py, pz, x, q);
}

void launch_ghost_fill_int(hipStream_t s, int nlocal, int nghost, int width, const int *owner, int *v) {
  const long long n = (long long)nghost * width;
  if (n <= 0) return;
  hipLaunchKernelGGL(ghost_fill_int_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, nlocal, n, width, owner, v);
}

void launch_ghost_fold(hipStream_t s, int nlocal, int width, const int *ofirst, const int *nimg, const int *list, double *v) {
  const long long n = (long long)nlocal * width;
  if (n <= 0) return;
  hipLaunchKernelGGL(ghost_fold_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, nlocal, width, ofirst, nimg, list, v);
}

void launch_atoms_wrap(hipStream_t s, const AtomsWrapArgs &a, double *x, int *image) {
  if (a.nlocal <= 0) return;
  hipLaunchKernelGGL(atoms_wrap_kernel, dim3((a.nlocal + 255) / 256), dim3(256), 0, s, a, x, image);
}

}  // namespace conp
