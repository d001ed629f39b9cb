// The transposed half list: a half list names each pair once, in its owner's row; to add an atom's forces
// without atomics the atom must also find the pairs in which it is the j.  For any flattened half list on the device:
//
//   own_row [nall]        the ii with ilist[ii] == a, or -1 (numneigh and first are valid for listed owners only: every row is
//                         reached through ilist)
//   tr_ptr  [nall + 1]    exclusive scan of the number of listed slots that name a
//   tr_entry[tr_ptr[nall]] for atom a, one int per slot p = first[i] + jj of a listed owner i with (neigh[p] & 0x3FFFFFFF) == a, in
//                         ASCENDING SLOT ORDER p: i | (neigh[p] & 0xC0000000), the owner with the special bits of that slot
//
//   tr_owners_kernel      own_row by compare-and-swap on the -1 the caller cleared it to: a second owner of a row raises the flag
//   tr_count_kernel       one wavefront per listed row, integer atomics count the members of every j (the result does not depend on
//                         the arrival order)
//   (conp_neigh.hip's scan) tr_ptr; tr_close_kernel stores tr_ptr[nall]
//   tr_fill_kernel        the same walk: a slot takes the next free place of its j's segment and stores (p << 32 | entry).  The
//                         place IS an arrival order -- it does not survive:
//   tr_sort_kernel        one wavefront per atom: an element's place is the number of keys of the segment below its own (slots are
//                         distinct: a permutation), any segment length.  The three arrays are a pure function of the list.
#include <hip/hip_runtime.h>

#include "conp_kernels.h"
#include "conp_transpose.hpp"

namespace conp {

namespace {

constexpr int TR_MASK = 0x3FFFFFFF;

__global__ __launch_bounds__(256) void tr_owners_kernel(TransposeArgs a, int *__restrict__ own_row, int *__restrict__ flag) {
  const int ii = blockIdx.x * 256 + threadIdx.x;
  if (ii >= a.inum) return;
  const int i = a.ilist[ii];
  if (i < 0 || i >= a.nall) { atomicOr(flag, 2); return; }
  if (atomicCAS(&own_row[i], -1, ii) != -1) atomicOr(flag, 1);
}

template <bool FILL>
__global__ __launch_bounds__(256) void tr_walk_kernel(TransposeArgs a, const int *__restrict__ tr_ptr, int *__restrict__ cnt,
                                                      long long *__restrict__ keys) {
  const int ii = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (ii >= a.inum) return;
  const int i = a.ilist[ii];
  if (i < 0 || i >= a.nall) return;              // (flagged by tr_owners_kernel: the build is refused)
  const int base = a.first[i], jn = a.numneigh[i];
  for (int jj = lane; jj < jn; jj += 64) {
    const int p = base + jj;
    const int raw = a.neigh[p];
    const int j = raw & TR_MASK;
    if (j >= a.nall) continue;                   // (conp_pair_set_list and the builds admit none; the fix's host list is not checked)
    const int place = atomicAdd(&cnt[j], 1);
    if (FILL) keys[(size_t)tr_ptr[j] + place] = ((long long)p << 32) | (long long)(unsigned)(i | (raw & ~TR_MASK));
  }
}

__global__ void tr_close_kernel(int nall, const long long *__restrict__ total, int *__restrict__ tr_ptr) { tr_ptr[nall] = (int)*total; }

__global__ __launch_bounds__(256) void tr_sort_kernel(int nall, const int *__restrict__ tr_ptr, const long long *__restrict__ keys,
                                                      int *__restrict__ tr_entry) {
  const int at = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (at >= nall) return;
  const int lo = tr_ptr[at], n = tr_ptr[at + 1] - lo;
  const long long *seg = keys + lo;
  for (int e = lane; e < n; e += 64) {
    const long long key = seg[e];
    int rank = 0;
    for (int k = 0; k < n; ++k) rank += seg[k] < key;
    tr_entry[(size_t)lo + rank] = (int)(unsigned)(key & 0xFFFFFFFFll);
  }
}

}  // namespace

void launch_tr_owners(hipStream_t s, const TransposeArgs &a, int *own_row, int *flag) {
  if (a.inum > 0) hipLaunchKernelGGL(tr_owners_kernel, dim3((a.inum + 255) / 256), dim3(256), 0, s, a, own_row, flag);
}

void launch_tr_count(hipStream_t s, const TransposeArgs &a, int *cnt) {
  if (a.inum > 0) hipLaunchKernelGGL((tr_walk_kernel<false>), dim3((a.inum + 3) / 4), dim3(256), 0, s, a, nullptr, cnt, nullptr);
}

void launch_tr_close(hipStream_t s, int nall, const long long *total, int *tr_ptr) {
  hipLaunchKernelGGL(tr_close_kernel, dim3(1), dim3(1), 0, s, nall, total, tr_ptr);
}

void launch_tr_fill(hipStream_t s, const TransposeArgs &a, const int *tr_ptr, int *cursor, long long *keys) {
  if (a.inum > 0) hipLaunchKernelGGL((tr_walk_kernel<true>), dim3((a.inum + 3) / 4), dim3(256), 0, s, a, tr_ptr, cursor, keys);
}

void launch_tr_sort(hipStream_t s, int nall, const int *tr_ptr, const long long *keys, int *tr_entry) {
  if (nall > 0) hipLaunchKernelGGL(tr_sort_kernel, dim3((nall + 3) / 4), dim3(256), 0, s, nall, tr_ptr, keys, tr_entry);
}

using namespace dev;

void TransposedList::build(const char *who, const TransposeArgs &a) {
  valid = false;                             // a refused build leaves no index
  if (a.nall < 0 || a.inum < 0) throw ConpError(CONP_ERR_ARG, std::string(who) + ": bad sizes");
  const size_t na = (size_t)std::max(a.nall, 1);
  ctx.sync();                                // no kernel may be reading the old index
  d_own_row.reserve(na); d_tr_ptr.reserve(na + 1); d_cnt.reserve(na); d_out.reserve(2);
  HIP_TRY(hipMemsetAsync(d_own_row.p, 0xFF, na * sizeof(int), ctx.stream));      // -1
  HIP_TRY(hipMemsetAsync(d_cnt.p, 0, na * sizeof(int), ctx.stream));
  HIP_TRY(hipMemsetAsync(d_out.p, 0, 2 * sizeof(long long), ctx.stream));
  launch_tr_owners(ctx.stream, a, d_own_row.p, reinterpret_cast<int *>(d_out.p + 1));
  launch_tr_count(ctx.stream, a, d_cnt.p);
  launch_neigh_scan(ctx.stream, a.nall, d_cnt.p, d_tr_ptr.p, d_out.p);
  launch_tr_close(ctx.stream, a.nall, d_out.p, d_tr_ptr.p);
  long long out[2] = {0, 0};
  HIP_TRY(hipMemcpyAsync(out, d_out.p, sizeof out, hipMemcpyDeviceToHost, ctx.stream));
  HIP_TRY(hipGetLastError());
  ctx.sync();
  const int flag = (int)(out[1] & 0xFFFFFFFFll);
  if (flag & 2) throw ConpError(CONP_ERR_ARG, std::string(who) + ": list owner outside [0, nall)");
  if (flag & 1) throw ConpError(CONP_ERR_ARG, std::string(who) + ": an owner occurs twice in ilist");
  if (out[0] >= (1ll << 31)) throw ConpError(CONP_ERR_NUMERIC, std::string(who) + ": 2^31 listed slots or more (tr_ptr is int)");
  const size_t ns = (size_t)std::max<long long>(out[0], 1);
  d_keys.reserve(ns); d_tr_entry.reserve(ns);
  HIP_TRY(hipMemsetAsync(d_cnt.p, 0, na * sizeof(int), ctx.stream));
  launch_tr_fill(ctx.stream, a, d_tr_ptr.p, d_cnt.p, d_keys.p);
  launch_tr_sort(ctx.stream, a.nall, d_tr_ptr.p, d_keys.p, d_tr_entry.p);
  HIP_TRY(hipGetLastError());
  ctx.sync();
  nall = a.nall; n = out[0];
  valid = true;
}

void TransposedList::get(const char *who, int *nall_, int64_t *n_, int *own_row, int *tr_ptr, int *tr_entry) {
  if (!valid) throw ConpError(CONP_ERR_STATE, std::string(who) + ": the handle has no transposed list of this kind");
  if (nall_) *nall_ = nall;
  if (n_) *n_ = n;
  if (own_row && nall > 0) HIP_TRY(hipMemcpyAsync(own_row, d_own_row.p, (size_t)nall * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
  if (tr_ptr) HIP_TRY(hipMemcpyAsync(tr_ptr, d_tr_ptr.p, ((size_t)nall + 1) * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
  if (tr_entry && n > 0) HIP_TRY(hipMemcpyAsync(tr_entry, d_tr_entry.p, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, ctx.stream));
  ctx.sync();
}

}  // namespace conp
