// The fix's re-neighbouring on the device -- conp_fix_post_neighbor_device of include/conp_hip.h, DESIGN.md section 19: what
// Fix::post_neighbor (conp_fix.cpp) forms on the host from the atom arrays, formed here from the handle's own ghost map (section 18)
// and the device arrays of the call.  Every table comes out in the order the host route gives it; nothing depends on which thread
// arrives first (the only atomics are the integer adds of the cell histogram, whose sums do not depend on their order).
//
//   ren_ghost_rows_kernel    type and atom -> electrode-row entry of every ghost copied from its owner
//   ren_compact_kernel       <FILL, PRED>: one wavefront per block of 64 atoms, four per workgroup; the atoms that pass PRED are ranked
//                            with a ballot and a popcount prefix.  The count pass writes count[block]; the fill pass -- the same code
//                            behind an exclusive scan (neigh_scan_kernel) -- writes the kept atoms in ascending index.
//                            PRED 0: atom2eleall >= 0 over all atoms -> the (atom, row) pairs of the charge scatter list;
//                            PRED 1: atom2eleall < 0 and q != 0 over the owned atoms -> the electrolyte list
//   ren_csr_count_kernel     per electrode row: its owned atom and 1 + the number of that atom's ghosts
//   ren_csr_fill_kernel      one thread per row: the owned atom, then its ghosts in ascending ghost index (the section-18 list)
//   ren_zcell_kernel         grid coordinate and cell of every listed atom (the host's expressions, no contraction), cell occupancy
//   ren_zsort_kernel         <FILL>: one workgroup per block of 256 listed atoms.  An atom's rank among the atoms of its block with
//                            the same key = (cell - start cell) mod n is the number of EARLIER ones (counted through LDS).  The count
//                            pass writes count[key][block]; the fill pass, behind the scan over (key, block), stores the atom at
//                            start[key][block] + rank: a stable counting sort.  It also stores the atom's first tap i0
//   ren_chunk_bounds_kernel  lowest and highest i0 of every chunk of 16 atoms of the sorted list
#include <hip/hip_runtime.h>

#include "conp_kernels.h"

namespace conp {

namespace {

__global__ __launch_bounds__(256) void ren_ghost_rows_kernel(int nlocal, int nghost, const int *__restrict__ owner, int *__restrict__ type,
                                                             int *__restrict__ a2e) {
  const int g = blockIdx.x * 256 + threadIdx.x;
  if (g >= nghost) return;
  const size_t o = (size_t)owner[g], i = (size_t)nlocal + g;
  type[i] = type[o];
  a2e[i] = a2e[o];
}

template <bool FILL, int PRED>
__global__ __launch_bounds__(256) void ren_compact_kernel(int n, int nblock, const int *__restrict__ a2e, const double *__restrict__ q,
                                                          int *__restrict__ count, const int *__restrict__ start, int cap,
                                                          int *__restrict__ out) {
  const int w = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (w >= nblock) return;                       // (whole waves leave; the kernel has no barrier)
  const int i = w * 64 + lane;
  int e = -1;
  bool keep = false;
  if (i < n) {
    e = a2e[i];
    keep = PRED == 0 ? e >= 0 : (e < 0 && q[i] != 0.0);
  }
  const unsigned long long vote = __ballot(keep);
  if (!FILL) {
    if (lane == 0) count[w] = __popcll(vote);
    return;
  }
  if (!keep) return;
  const int k = start[w] + __popcll(vote & ((1ull << lane) - 1ull));
  if (k >= cap) return;                          // (what the count pass found: the fill pass never stores past it)
  if (PRED == 0) { out[2 * (size_t)k] = i; out[2 * (size_t)k + 1] = e; }
  else out[k] = i;
}

__global__ __launch_bounds__(256) void ren_csr_count_kernel(int nlocal, int ne, const int *__restrict__ a2e, const int *__restrict__ nimg,
                                                            int *__restrict__ own_of, int *__restrict__ cnt) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nlocal) return;
  const int e = a2e[i];
  if (e < 0 || e >= ne) return;
  own_of[e] = i;
  cnt[e] = 1 + (nimg ? nimg[i] : 0);
}

__global__ __launch_bounds__(256) void ren_csr_fill_kernel(int nlocal, int ne, int cap, const int *__restrict__ own_of, const int *__restrict__ ptr,
                                                           const int *__restrict__ ofirst, const int *__restrict__ nimg,
                                                           const int *__restrict__ list, int *__restrict__ of, int *__restrict__ rowof) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= ne) return;
  int k = ptr[r];
  const int end = min(ptr[r + 1], cap);
  if (k >= end) return;                          // (a row without an owned atom: not on a handle this entry accepts)
  const int o = own_of[r];
  of[k] = o; rowof[k] = r;
  ++k;
  if (!nimg) return;
  const int b = ofirst[o];
  for (int m = 0; k < end; ++m, ++k) { of[k] = nlocal + list[b + m]; rowof[k] = r; }
}

__global__ __launch_bounds__(256) void ren_zcell_kernel(ZnOrderArgs a, const long long *__restrict__ nl_dev, const int *__restrict__ list,
                                                        const double *__restrict__ x, int *__restrict__ cell, double *__restrict__ uw,
                                                        int *__restrict__ occ) {
#pragma clang fp contract(off)
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= (int)*nl_dev) return;
  double u = x[3 * (size_t)list[k] + 2] * a.gscale;
  u -= a.n * floor(u * a.rn);
  int c = (int)u;
  if (c >= a.n) { c = a.n - 1; u = a.n_below; }
  if (c < 0) c = 0;                              // (a coordinate that is not a number: the host's conversion is undefined there)
  uw[k] = u; cell[k] = c;
  atomicAdd(&occ[c], 1);
}

template <bool FILL>
__global__ __launch_bounds__(256) void ren_zsort_kernel(ZnOrderArgs a, int nl, int nblock, int c_start, const int *__restrict__ list,
                                                        const int *__restrict__ cell, const double *__restrict__ uw, int *__restrict__ count,
                                                        const int *__restrict__ start, int *__restrict__ sorted, int *__restrict__ i0s) {
#pragma clang fp contract(off)
  __shared__ int key_s[256];
  const int b = blockIdx.x, t = threadIdx.x, k = b * 256 + t;
  const int nvalid = min(256, nl - b * 256);
  int key = 0;
  if (t < nvalid) {
    key = cell[k] - c_start;
    if (key < 0) key += a.n;
  }
  key_s[t] = key;
  __syncthreads();
  if (t >= nvalid) return;
  int before = 0, all = 0;
  for (int j = 0; j < nvalid; ++j) {             // (every lane reads the same word: a broadcast)
    const int same = key_s[j] == key;
    all += same;
    before += same && j < t;
  }
  const size_t e = (size_t)key * nblock + b;
  if (!FILL) {
    if (before == all - 1) count[e] = all;       // the last atom of its key in this block; the others' entries stay zero
    return;
  }
  const int pos = start[e] + before;
  if (pos >= nl) return;
  sorted[pos] = list[k];
  double ur = uw[k] - c_start;
  if (ur < 0.0) ur += a.n;
  i0s[pos] = (int)ceil(ur - 0.5 * a.w);
}

__global__ __launch_bounds__(256) void ren_chunk_bounds_kernel(int nl, int nch, const int *__restrict__ i0s, int *__restrict__ lo,
                                                               int *__restrict__ hi) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c >= nch) return;
  int l = 0x3fffffff, h = -0x3fffffff;
  const int end = min(nl, 16 * c + 16);
  for (int k = 16 * c; k < end; ++k) { const int v = i0s[k]; l = min(l, v); h = max(h, v); }
  lo[c] = l; hi[c] = h;
}

}  // namespace

void launch_ren_ghost_rows(hipStream_t s, int nlocal, int nghost, const int *owner, int *type, int *a2e) {
  if (nghost <= 0) return;
  hipLaunchKernelGGL(ren_ghost_rows_kernel, dim3((nghost + 255) / 256), dim3(256), 0, s, nlocal, nghost, owner, type, a2e);
}

void launch_ren_compact(hipStream_t s, int pred, bool fill, int n, const int *a2e, const double *q, int *count, const int *start, int cap,
                        int *out) {
  const int nblock = (n + 63) / 64;
  if (nblock <= 0) return;
  const dim3 grid((nblock + 3) / 4), block(256);
  if (pred == 0) {
    if (fill) hipLaunchKernelGGL((ren_compact_kernel<true, 0>), grid, block, 0, s, n, nblock, a2e, q, count, start, cap, out);
    else hipLaunchKernelGGL((ren_compact_kernel<false, 0>), grid, block, 0, s, n, nblock, a2e, q, count, start, cap, out);
  } else {
    if (fill) hipLaunchKernelGGL((ren_compact_kernel<true, 1>), grid, block, 0, s, n, nblock, a2e, q, count, start, cap, out);
    else hipLaunchKernelGGL((ren_compact_kernel<false, 1>), grid, block, 0, s, n, nblock, a2e, q, count, start, cap, out);
  }
}

void launch_ren_csr_count(hipStream_t s, int nlocal, int ne, const int *a2e, const int *nimg, int *own_of, int *cnt) {
  if (nlocal <= 0) return;
  hipLaunchKernelGGL(ren_csr_count_kernel, dim3((nlocal + 255) / 256), dim3(256), 0, s, nlocal, ne, a2e, nimg, own_of, cnt);
}

void launch_ren_csr_fill(hipStream_t s, int nlocal, int ne, int cap, const int *own_of, const int *ptr, const int *ofirst, const int *nimg,
                         const int *list, int *of, int *rowof) {
  if (ne <= 0) return;
  hipLaunchKernelGGL(ren_csr_fill_kernel, dim3((ne + 255) / 256), dim3(256), 0, s, nlocal, ne, cap, own_of, ptr, ofirst, nimg, list, of, rowof);
}

void launch_ren_zcell(hipStream_t s, const ZnOrderArgs &a, int nl_max, const long long *nl_dev, const int *list, const double *x, int *cell,
                      double *uw, int *occ) {
  if (nl_max <= 0) return;
  hipLaunchKernelGGL(ren_zcell_kernel, dim3((nl_max + 255) / 256), dim3(256), 0, s, a, nl_dev, list, x, cell, uw, occ);
}

void launch_ren_zsort(hipStream_t s, const ZnOrderArgs &a, bool fill, int nl, int c_start, const int *list, const int *cell, const double *uw,
                      int *count, const int *start, int *sorted, int *i0s) {
  const int nblock = (nl + 255) / 256;
  if (nblock <= 0) return;
  if (fill) hipLaunchKernelGGL(ren_zsort_kernel<true>, dim3(nblock), dim3(256), 0, s, a, nl, nblock, c_start, list, cell, uw, count, start, sorted, i0s);
  else hipLaunchKernelGGL(ren_zsort_kernel<false>, dim3(nblock), dim3(256), 0, s, a, nl, nblock, c_start, list, cell, uw, count, start, sorted, i0s);
}

void launch_ren_chunk_bounds(hipStream_t s, int nl, const int *i0s, int *lo, int *hi) {
  const int nch = (nl + 15) / 16;
  if (nch <= 0) return;
  hipLaunchKernelGGL(ren_chunk_bounds_kernel, dim3((nch + 255) / 256), dim3(256), 0, s, nl, nch, i0s, lo, hi);
}

}  // namespace conp
