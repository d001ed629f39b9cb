// The pair style's half neighbour list built on the device from d_x -- conp_pair_build_list_device / conp_pair_list_moved_device of
// include/conp_hip.h, DESIGN.md section 17.  The list is the one conp_amd/neighbor.py::_half_pairs defines (LAMMPS half/bin/newtoff
// and half/bin/newton as a set), with LAMMPS' special-bond bits; the result is a pure function of the input: no order in it depends
// on which atomic arrives first.
//
//   neigh_extent_kernel   one workgroup: lower and upper bound of x[0 .. nall) per dimension, and whether every coordinate is finite
//   neigh_cell_kernel     cell of every atom (clamped into the grid), members counted per cell.  The slot the counting atomic hands
//                         out is an arrival order: it only places the atom in the UNSORTED member array
//   neigh_scan_kernel     one workgroup: exclusive scan of an int array, 64-bit total (cell starts; `first` from numneigh)
//   neigh_scatter_kernel  unsorted[start[cell] + slot] = atom
//   neigh_sort_kernel     one workgroup per cell: a member's place is the number of members with a smaller index (indices are
//                         distinct: a permutation) -> members ascending by atom index, stored as (x, y, z, index) records
//   neigh_row_kernel      <FILL, SPECIAL, EXCLUDE> (EXCLUDE: with the exclusion test of section 25): one wavefront per owner, four per workgroup.  The 27 cells around the owner's are walked in
//                         a fixed order, lanes stride over a cell's members and test the pair; accepted entries are compacted with a
//                         ballot and a popcount prefix, so a row's order is the traversal order.  The count pass writes numneigh, the
//                         fill pass the entries: the same code
//   neigh_iota_kernel     ilist = 0 .. nlocal-1
//   neigh_moved_kernel    one workgroup, one reduction: flag = any owned atom further than `trigger` from its place at the build
#include <hip/hip_runtime.h>

#include <type_traits>

#include "conp_kernels.h"

namespace conp {

namespace {

__device__ __forceinline__ bool neigh_finite(double v) { return fabs(v) <= 1.79769313486231570815e308; }   // false for NaN, +-inf

// cell index of coordinate v along one dimension: NaN and everything below the lower bound go to cell 0, everything at or above
// the upper bound -- the atom that defines it included -- to the last cell
__device__ __forceinline__ int neigh_cell_of(double v, double lo, double inv, int n) {
  const double t = (v - lo) * inv;
  if (!(t >= 0.0)) return 0;
  if (!(t < (double)n)) return n - 1;
  const int c = (int)t;
  return c < n ? c : n - 1;
}

__global__ __launch_bounds__(1024) void neigh_extent_kernel(int nall, const double *__restrict__ x, double *__restrict__ ext) {
  __shared__ double lo_s[16][3], hi_s[16][3];
  __shared__ int bad_s[16];
  double lo[3] = {1.79769313486231570815e308, 1.79769313486231570815e308, 1.79769313486231570815e308};
  double hi[3] = {-1.79769313486231570815e308, -1.79769313486231570815e308, -1.79769313486231570815e308};
  int bad = 0;
  for (int i = threadIdx.x; i < nall; i += 1024) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double v = x[3 * (size_t)i + c];
      if (!neigh_finite(v)) bad = 1;
      else { lo[c] = fmin(lo[c], v); hi[c] = fmax(hi[c], v); }
    }
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lo[c] = fmin(lo[c], __shfl_down(lo[c], off, 64));
      hi[c] = fmax(hi[c], __shfl_down(hi[c], off, 64));
    }
    bad |= __shfl_down(bad, off, 64);
  }
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) { lo_s[w][c] = lo[c]; hi_s[w][c] = hi[c]; }
    bad_s[w] = bad;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 16; ++k) {
#pragma unroll
      for (int c = 0; c < 3; ++c) { lo[c] = fmin(lo[c], lo_s[k][c]); hi[c] = fmax(hi[c], hi_s[k][c]); }
      bad |= bad_s[k];
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) { ext[c] = lo[c]; ext[3 + c] = hi[c]; }
    ext[6] = bad ? 1.0 : 0.0;
  }
}

__global__ __launch_bounds__(256) void neigh_cell_kernel(int nall, const double *__restrict__ x, NeighGrid g, int *__restrict__ cell,
                                                         int *__restrict__ slot, int *__restrict__ count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nall) return;
  const int cx = neigh_cell_of(x[3 * (size_t)i], g.lo[0], g.inv[0], g.n[0]);
  const int cy = neigh_cell_of(x[3 * (size_t)i + 1], g.lo[1], g.inv[1], g.n[1]);
  const int cz = neigh_cell_of(x[3 * (size_t)i + 2], g.lo[2], g.inv[2], g.n[2]);
  const int c = (cz * g.n[1] + cy) * g.n[0] + cx;
  cell[i] = c;
  slot[i] = atomicAdd(&count[c], 1);
}

// out[k] = in[0] + .. + in[k-1] for k < n (as int: the caller refuses a total that does not fit), *total = the 64-bit sum.
// out_end != 0: out[n] = the total as well.
__global__ __launch_bounds__(1024) void neigh_scan_kernel(int n, const int *__restrict__ in, int *__restrict__ out, int out_end,
                                                          long long *__restrict__ total) {
  __shared__ long long wsum[16];
  __shared__ long long carry_s;
  if (threadIdx.x == 0) carry_s = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int base = 0; base < n; base += 1024) {
    const int k = base + threadIdx.x;
    const long long v = k < n ? (long long)in[k] : 0;
    long long inc = v;                              // inclusive scan inside the wave
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
      const long long t = __shfl_up(inc, off, 64);
      if (lane >= off) inc += t;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    long long before = carry_s;
    for (int k2 = 0; k2 < w; ++k2) before += wsum[k2];
    if (k < n) out[k] = (int)(before + inc - v);
    __syncthreads();
    if (threadIdx.x == 1023) carry_s = before + inc;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    if (out_end) out[n] = (int)carry_s;
    *total = carry_s;
  }
}

__global__ __launch_bounds__(256) void neigh_scatter_kernel(int nall, const int *__restrict__ cell, const int *__restrict__ slot,
                                                            const int *__restrict__ start, int *__restrict__ unsorted) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nall) return;
  unsorted[start[cell[i]] + slot[i]] = i;
}

__global__ __launch_bounds__(256) void neigh_sort_kernel(const int *__restrict__ start, const int *__restrict__ unsorted,
                                                         const double *__restrict__ x, double4 *__restrict__ sorted) {
  const int s = start[blockIdx.x], e = start[blockIdx.x + 1];
  for (int m = s + threadIdx.x; m < e; m += 256) {
    const int me = unsorted[m];
    int rank = 0;
    for (int k = s; k < e; ++k) rank += unsorted[k] < me;
    sorted[s + rank] = make_double4(x[3 * (size_t)me], x[3 * (size_t)me + 1], x[3 * (size_t)me + 2], (double)me);
  }
}

// Neighbor::exclusion(i, j, ..) of LAMMPS for one candidate: the owner's class data are wave-uniform, the candidate's are gathered
// by the lanes that already pass the distance and orientation tests (variant (a))
__device__ __forceinline__ bool neigh_excluded(const NeighExclArgs &ex, int ti, int mi, int moli, int j) {
  if (ex.ntype) {
    const int tj = min(max(ex.type[j], 0), ex.nt1 - 1);
    if (ex.ex_type[ti * ex.nt1 + tj]) return true;
  }
  if (ex.ngroup | ex.nmol) {
    const int mj = ex.mask[j];
    for (int m = 0; m < ex.ngroup; ++m) {
      if ((mi & ex.gbit1[m]) && (mj & ex.gbit2[m])) return true;
      if ((mi & ex.gbit2[m]) && (mj & ex.gbit1[m])) return true;
    }
    if (ex.nmol) {
      const int molj = ex.molecule[j];
      for (int m = 0; m < ex.nmol; ++m)
        if ((mi & ex.mbit[m]) && (mj & ex.mbit[m])) {
          if ((ex.mintra >> m) & 1u) { if (moli == molj) return true; }
          else if (moli != molj) return true;
        }
    }
  }
  return false;
}

struct NeighNoExcl {};                           // the second argument of the instantiations without the exclusion test

template <bool FILL, bool SPECIAL, bool EXCLUDE>
__global__ __launch_bounds__(256) void neigh_row_kernel(NeighRowArgs a, std::conditional_t<EXCLUDE, NeighExclArgs, NeighNoExcl> ex) {
#pragma clang fp contract(off)
  const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (i >= a.nlocal) return;                     // (whole waves leave; the kernel has no barrier)
  const double xi = a.x[3 * (size_t)i], yi = a.x[3 * (size_t)i + 1], zi = a.x[3 * (size_t)i + 2];
  const int c = a.cell[i];
  const int nx = a.g.n[0], ny = a.g.n[1], nz = a.g.n[2];
  const int cx = c % nx, cy = (c / nx) % ny, cz = c / (nx * ny);
  int n1 = 0, n2 = 0, n3 = 0;
  const int *spec = nullptr;
  if (SPECIAL) {                                 // cumulative counts, kept inside [0, maxspecial] whatever the table holds
    n3 = min(max(a.nspecial[3 * (size_t)i + 2], 0), a.maxspecial);
    n2 = min(max(a.nspecial[3 * (size_t)i + 1], 0), n3);
    n1 = min(max(a.nspecial[3 * (size_t)i], 0), n2);
    spec = a.special + (size_t)i * a.maxspecial;
  }
  int ti = 0, mi = 0, moli = 0;                  // EXCLUDE: the owner's type (clamped into the table), mask and molecule id
  if constexpr (EXCLUDE) {
    if (ex.ntype) ti = min(max(ex.type[i], 0), ex.nt1 - 1);
    if (ex.ngroup | ex.nmol) mi = ex.mask[i];
    if (ex.nmol) moli = ex.molecule[i];
  }
  int *row = FILL ? a.neigh + a.first[i] : nullptr;
  const int room = FILL ? a.numneigh[i] : 0;     // what the count pass found: the fill pass never stores past it
  const unsigned long long below = (1ull << lane) - 1ull;
  int base = 0;
  for (int dz = -1; dz <= 1; ++dz) {
    const int z = cz + dz;
    if (z < 0 || z >= nz) continue;
    for (int dy = -1; dy <= 1; ++dy) {
      const int y = cy + dy;
      if (y < 0 || y >= ny) continue;
      for (int dx = -1; dx <= 1; ++dx) {
        const int xc = cx + dx;
        if (xc < 0 || xc >= nx) continue;
        const int cc = (z * ny + y) * nx + xc;
        const int s = a.start[cc], e = a.start[cc + 1];
        for (int m0 = s; m0 < e; m0 += 64) {     // the trip count is the same for every lane: the ballot sees the whole wave
          const int m = m0 + lane;
          bool keep = false;
          int entry = 0;
          if (m < e) {
            const double4 p = a.sorted[m];
            const int j = (int)p.w;
            const double delx = xi - p.x, dely = yi - p.y, delz = zi - p.z;
            const double rsq = delx * delx + dely * dely + delz * delz;
            if (rsq < a.cutneighsq) {
              if (j < a.nlocal || !a.newton) keep = j > i;
              else keep = p.z > zi || (p.z == zi && (p.y > yi || (p.y == yi && p.x > xi)));
            }
            entry = j;
            if constexpr (EXCLUDE) {
              if (keep) keep = !neigh_excluded(ex, ti, mi, moli, j);           // a dropped pair is absent: it votes 0
            }
            if (SPECIAL && keep) {
              const int tj = a.tag[j];
              int pos = -1;
              for (int k = 0; k < n3; ++k)
                if (spec[k] == tj) { pos = k; break; }
              if (pos >= 0) {
                const int which = pos < n1 ? 1 : (pos < n2 ? 2 : 3);
                const bool image = (a.prd_half[0] > 0.0 && fabs(delx) > a.prd_half[0]) || (a.prd_half[1] > 0.0 && fabs(dely) > a.prd_half[1]) ||
                                   (a.prd_half[2] > 0.0 && fabs(delz) > a.prd_half[2]);
                if (a.flagged[which] && !image) entry = (int)((unsigned)j | ((unsigned)which << 30));
              }
            }
          }
          const unsigned long long vote = __ballot(keep);
          if (FILL && keep) {
            const int at = base + __popcll(vote & below);
            if (at < room) row[at] = entry;
          }
          base += __popcll(vote);
        }
      }
    }
  }
  if (!FILL && lane == 0) a.numneigh[i] = base;
}

__global__ __launch_bounds__(256) void neigh_iota_kernel(int n, int *__restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) out[i] = i;
}

__global__ __launch_bounds__(1024) void neigh_moved_kernel(int nlocal, const double *__restrict__ x, const double *__restrict__ xb,
                                                           double trigsq, int *__restrict__ flag) {
#pragma clang fp contract(off)
  __shared__ int any_s[16];
  int any = 0;
  for (int i = threadIdx.x; i < nlocal; i += 1024) {
    const double dx = x[3 * (size_t)i] - xb[3 * (size_t)i], dy = x[3 * (size_t)i + 1] - xb[3 * (size_t)i + 1],
                 dz = x[3 * (size_t)i + 2] - xb[3 * (size_t)i + 2];
    if (!(dx * dx + dy * dy + dz * dz <= trigsq)) any = 1;      // (a NaN coordinate counts as moved: the build that follows refuses it)
  }
  any = __ballot(any != 0) != 0ull;
  if ((threadIdx.x & 63) == 0) any_s[threadIdx.x >> 6] = any;
  __syncthreads();
  if (threadIdx.x == 0) {
    for (int k = 1; k < 16; ++k) any |= any_s[k];
    *flag = any;
  }
}

template <bool FILL>
void launch_neigh_rows_t(hipStream_t s, const NeighRowArgs &a) {
  const dim3 grid((a.nlocal + 3) / 4), block(256);
  if (a.tag) hipLaunchKernelGGL((neigh_row_kernel<FILL, true, false>), grid, block, 0, s, a, NeighNoExcl{});
  else hipLaunchKernelGGL((neigh_row_kernel<FILL, false, false>), grid, block, 0, s, a, NeighNoExcl{});
}

template <bool FILL>
void launch_neigh_rows_exclude_t(hipStream_t s, const NeighRowArgs &a, const NeighExclArgs &ex) {
  const dim3 grid((a.nlocal + 3) / 4), block(256);
  if (a.tag) hipLaunchKernelGGL((neigh_row_kernel<FILL, true, true>), grid, block, 0, s, a, ex);
  else hipLaunchKernelGGL((neigh_row_kernel<FILL, false, true>), grid, block, 0, s, a, ex);
}

}  // namespace

void launch_neigh_extent(hipStream_t s, int nall, const double *x, double *ext) {
  hipLaunchKernelGGL(neigh_extent_kernel, dim3(1), dim3(1024), 0, s, nall, x, ext);
}

void launch_neigh_bin(hipStream_t s, int nall, const double *x, const NeighGrid &g, int *cell, int *slot, int *count, int *start,
                      long long *total, int *unsorted, double4 *sorted) {
  const int ncell = g.n[0] * g.n[1] * g.n[2];
  const dim3 grid((nall + 255) / 256), block(256);
  (void)hipMemsetAsync(count, 0, (size_t)ncell * sizeof(int), s);
  if (nall > 0) hipLaunchKernelGGL(neigh_cell_kernel, grid, block, 0, s, nall, x, g, cell, slot, count);
  hipLaunchKernelGGL(neigh_scan_kernel, dim3(1), dim3(1024), 0, s, ncell, count, start, 1, total);
  if (nall > 0) {
    hipLaunchKernelGGL(neigh_scatter_kernel, grid, block, 0, s, nall, cell, slot, start, unsorted);
    hipLaunchKernelGGL(neigh_sort_kernel, dim3(ncell), block, 0, s, start, unsorted, x, sorted);
  }
}

void launch_neigh_rows(hipStream_t s, const NeighRowArgs &a, bool fill) {
  if (a.nlocal <= 0) return;
  if (fill) launch_neigh_rows_t<true>(s, a);
  else launch_neigh_rows_t<false>(s, a);
}

void launch_neigh_rows_exclude(hipStream_t s, const NeighRowArgs &a, const NeighExclArgs &ex, bool fill) {
  if (a.nlocal <= 0) return;
  if (fill) launch_neigh_rows_exclude_t<true>(s, a, ex);
  else launch_neigh_rows_exclude_t<false>(s, a, ex);
}

void launch_neigh_scan(hipStream_t s, int n, const int *in, int *out, long long *total) {
  hipLaunchKernelGGL(neigh_scan_kernel, dim3(1), dim3(1024), 0, s, n, in, out, 0, total);
}

void launch_neigh_iota(hipStream_t s, int n, int *out) {
  if (n > 0) hipLaunchKernelGGL(neigh_iota_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, out);
}

void launch_neigh_moved(hipStream_t s, int nlocal, const double *x, const double *xb, double trigsq, int *flag) {
  hipLaunchKernelGGL(neigh_moved_kernel, dim3(1), dim3(1024), 0, s, nlocal, x, xb, trigsq, flag);
}

}  // namespace conp
