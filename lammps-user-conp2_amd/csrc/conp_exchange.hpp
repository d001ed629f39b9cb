// struct RankExchange: what a handle knows about several ranks -- the host's conp_comm callbacks (spatially decomposed atoms, ranks
// that share a GPU), an RCCL communicator (one rank per GPU, collectives on the handle's stream), and the two device exchanges
// every call site is made of: sum() and gather_rows() (conp_exchange.cpp).
#pragma once
#include "conp_host.hpp"
#include "conp_dev.hpp"

struct ncclComm;      // rccl.h's communicator: only conp_exchange.cpp reads that header

namespace conp {

// ---- ranks: the host's conp_comm callbacks behind the RankOps interface of conp_host.hpp ----------------------------------
struct RankComm : RankOps {
  conp_comm c{};
  bool have = false;            // callbacks present: the atoms handed to the hooks are this rank's sub-domain
  int rank_ = 0, nranks_ = 1;
  int nranks() const override { return nranks_; }
  int rank() const override { return rank_; }
  bool active() const { return have && nranks_ > 1; }
  static void check(int rc, const char *what) {
    if (rc != 0) throw dev::ConpError(CONP_ERR_STATE, std::string("conp_comm callback failed: ") + what);
  }
  void allreduce_max_int(int *v, int n) override { if (active()) check(c.allreduce_max_int(c.ctx, v, n), "allreduce_max_int"); }
  void allgather_int(int v, int *out) override {
    if (active()) check(c.allgather_int(c.ctx, v, out), "allgather_int"); else out[0] = v;
  }
  void allgatherv_int(const int *send, int n, int *recv, const int *counts, const int *displs) override {
    if (!active()) { for (int i = 0; i < n; ++i) recv[i] = send[i]; return; }
    std::vector<int64_t> cb(nranks_), db(nranks_);
    for (int r = 0; r < nranks_; ++r) { cb[r] = (int64_t)counts[r] * sizeof(int); db[r] = (int64_t)displs[r] * sizeof(int); }
    check(c.allgatherv(c.ctx, send, (int64_t)n * sizeof(int), recv, cb.data(), db.data()), "allgatherv");
  }
  void sum(double *b, int64_t n) override { if (active() && n > 0) check(c.allreduce_sum(c.ctx, b, n), "allreduce_sum"); }
  void gatherv(const double *send, const std::vector<int> &items, int w, double *recv) override {
    if (!active()) { std::memcpy(recv, send, (size_t)items[0] * w * sizeof(double)); return; }
    std::vector<int64_t> cb(nranks_), db(nranks_);
    int64_t off = 0;
    for (int r = 0; r < nranks_; ++r) { cb[r] = (int64_t)items[r] * w * sizeof(double); db[r] = off; off += cb[r]; }
    check(c.allgatherv(c.ctx, send, cb[rank_], recv, cb.data(), db.data()), "allgatherv");
  }
};

struct RankExchange {
  explicit RankExchange(dev::DevCtx &c) : ctx(c) {}
  ~RankExchange() { destroy_rccl(); }      // nothing left to do where the handle gave the communicator back before its stream went
  dev::DevCtx &ctx;                        // the handle's stream (read at every call: conp_fix_set_stream may replace it) and wait
  RankComm cb;                             // what EleIndex, EwaldQuery::ranks and PppmMesh::ranks receive as RankOps *
  bool decomposed = false;                 // conp_fix_set_comm was called: atoms and lists are this rank's sub-domain

  bool has_comm() const { return comm != nullptr; }      // an RCCL communicator (of one rank too: how a one-GPU box tests the calls)
  bool callbacks_active() const { return cb.active(); }
  // any way to exchange at all: the setup shards A and S then, the host hooks sum b then.  (No test of conp_env.nranks beside it:
  // conp_fix_set_comm sets it to cb.nranks_ and nothing changes either afterwards, so cb.active() already says nranks > 1.)
  bool can_exchange() const { return has_comm() || cb.active(); }
  // the device-resident entries take replicated atoms: CONP_ERR_STATE on a decomposed handle
  void need_replicated() const;

  // conp_fix_set_comm, conp_rccl_unique_id, conp_rccl_available, conp_fix_comm_init_rccl, conp_fix_comm_destroy_rccl
  void set_callbacks(const conp_comm *comm);
  static void unique_id(void *id_out);
  static bool available();
  void init_rccl(const void *id, int nranks, int rank);      // collective; the handle's device is the thread's current one
  void destroy_rccl();                                       // waits for the stream first; no-op without a communicator

  // In-place all-reduce of the n doubles at d (device): RCCL on the stream, else the callbacks through stage -- host memory for n
  // doubles that stays the caller's until the stream has drained (the upload back is enqueued, not waited for; RCCL leaves stage
  // untouched).  what: the RCCL error's label.  CONP_ERR_STATE where there is neither communicator nor callbacks.
  void sum(double *d, size_t n, double *stage, const char *what);
  // All-gather of the ranks' row blocks of d_full [ne][width] (device): rank r holds rows [min(ne, r rows_per), min(ne, (r + 1)
  // rows_per)) at their place.  RCCL gathers rows_per * width doubles per rank in place (d_full holds nranks * rows_per rows);
  // the callbacks go through stage, host memory for (ne + rows_per) * width doubles: the whole first, the own block behind it.
  // Enqueues the upload back like sum(); without communicator or callbacks d_full is left as it is.
  void gather_rows(double *d_full, int ne, int rows_per, int width, double *stage, const char *what);

 private:
  ncclComm *comm = nullptr;
  int comm_rank = 0;                       // this rank's slot in the communicator
};

}  // namespace conp
