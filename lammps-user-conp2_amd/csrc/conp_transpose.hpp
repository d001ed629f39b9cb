// struct TransposedList: the index that lets an atom find the pairs of a half list in which it is the j (conp_transpose.hip,
// DESIGN.md section 26).  One per list: the pair style's and the fix's own.
#pragma once
#include "conp_dev.hpp"
#include "conp_kernels.h"

namespace conp {

struct TransposedList {
  dev::DevCtx &ctx;                                                     // the handle's stream and wait
  bool valid = false;                     // cleared by whatever replaces the list the index was built from
  int nall = 0;
  int64_t n = 0;                          // listed slots: tr_ptr[nall]
  dev::DevBuf<int> d_own_row, d_tr_ptr, d_tr_entry, d_cnt;
  dev::DevBuf<long long> d_keys, d_out;   // d_out: [0] the slot count, [1] the refusal flags of the owner pass

  explicit TransposedList(dev::DevCtx &c) : ctx(c) {}
  // may allocate and synchronise (the slot count reaches the host to size tr_entry); a refused build leaves no index
  void build(const char *who, const TransposeArgs &a);
  void get(const char *who, int *nall_, int64_t *n_, int *own_row, int *tr_ptr, int *tr_entry);
  TransposedView view() const { return TransposedView{d_own_row.p, d_tr_ptr.p, d_tr_entry.p, nall}; }
};

}  // namespace conp
