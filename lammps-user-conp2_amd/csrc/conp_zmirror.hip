// `fix zmirror` on the device -- conp_zmirror_post_integrate_device of include/conp_hip.h, DESIGN.md section 25.  One thread per
// (source, target) pair copies the source's x and y and reflects its z: x[dst] = (x[src][0], x[src][1], zoffset - x[src][2]).  No
// target is a source (conp_zmirror_set_params refuses that), so the copy in place equals the reference's snapshot-then-write.
#include <hip/hip_runtime.h>

#include "conp_kernels.h"

namespace conp {

namespace {

__global__ __launch_bounds__(ZMIRROR_BLOCK) void zmirror_kernel(int npairs, const int2 *__restrict__ map, double zoffset,
                                                                 double *__restrict__ x) {
  const int k = blockIdx.x * ZMIRROR_BLOCK + threadIdx.x;
  if (k >= npairs) return;
  const int2 p = map[k];
  const size_t s = 3 * (size_t)p.x, d = 3 * (size_t)p.y;
  const double xs = x[s], ys = x[s + 1], zs = x[s + 2];
  x[d] = xs;
  x[d + 1] = ys;
  x[d + 2] = zoffset - zs;
}

}  // namespace

void launch_zmirror(hipStream_t s, int npairs, const int2 *map, double zoffset, double *x) {
  if (npairs > 0) hipLaunchKernelGGL(zmirror_kernel, dim3((npairs + ZMIRROR_BLOCK - 1) / ZMIRROR_BLOCK), dim3(ZMIRROR_BLOCK), 0, s, npairs, map, zoffset, x);
}

}  // namespace conp
