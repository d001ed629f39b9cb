// The exchanges between the ranks of one `fix conp`: RCCL on the handle's stream when a communicator exists
// (one rank per GPU), else the host's callbacks through host staging memory (ranks that share a GPU, the LAMMPS glue's default).
// MPI_Allgatherv + MPI_Allreduce of the reference: fix_conp.cpp:643 (b_comm of b and of q), :1356 (newtonbuf).
#include "conp_exchange.hpp"

#include <dlfcn.h>
#include <rccl/rccl.h>   // types and enums only: the entry points are resolved with dlopen when a communicator is asked for

namespace conp {
using namespace dev;
namespace {

// ---- RCCL, resolved at run time (the library stays loadable where no RCCL is installed; torch's bundled copy and the
// system's share a soname, whichever the process loaded first serves both) -------------------------------------------------
struct Rccl {
  void *lib = nullptr;
  ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
  ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
  ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
  ncclResult_t (*AllReduce)(const void *, void *, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  const char *(*GetErrorString)(ncclResult_t) = nullptr;
  void load() {
    if (lib) return;
    for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      lib = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (lib) break;
    }
    if (!lib) throw ConpError(CONP_ERR_NO_DEVICE, std::string("cannot load librccl: ") + dlerror());
    auto sym = [&](const char *n) {
      void *p = dlsym(lib, n);
      if (!p) throw ConpError(CONP_ERR_NO_DEVICE, std::string("librccl lacks ") + n);
      return p;
    };
    GetUniqueId = reinterpret_cast<decltype(GetUniqueId)>(sym("ncclGetUniqueId"));
    CommInitRank = reinterpret_cast<decltype(CommInitRank)>(sym("ncclCommInitRank"));
    CommDestroy = reinterpret_cast<decltype(CommDestroy)>(sym("ncclCommDestroy"));
    AllReduce = reinterpret_cast<decltype(AllReduce)>(sym("ncclAllReduce"));
    AllGather = reinterpret_cast<decltype(AllGather)>(sym("ncclAllGather"));
    GetErrorString = reinterpret_cast<decltype(GetErrorString)>(sym("ncclGetErrorString"));
  }
  void ok(ncclResult_t r, const char *what) {
    if (r != ncclSuccess) throw ConpError(CONP_ERR_NO_DEVICE, std::string("RCCL error in ") + what + ": " + (GetErrorString ? GetErrorString(r) : "?"));
  }
};
Rccl g_rccl;   // plain pointers, no destructor: nothing of it runs at exit

}  // namespace

void RankExchange::need_replicated() const {
  if (decomposed) throw ConpError(CONP_ERR_STATE, "device-resident updates take replicated atoms (conp_env.rank / nranks); "
                                                  "spatially decomposed runs use the host-buffer hooks");
}

void RankExchange::set_callbacks(const conp_comm *comm) {
  if (comm->nranks < 1 || comm->rank < 0 || comm->rank >= comm->nranks) throw ConpError(CONP_ERR_ARG, "bad rank/nranks");
  if (comm->nranks > 1 && (!comm->allreduce_sum || !comm->allreduce_max_int || !comm->allgather_int || !comm->allgatherv))
    throw ConpError(CONP_ERR_ARG, "conp_comm: every callback is needed with more than one rank");
  cb.c = *comm; cb.have = true; cb.rank_ = comm->rank; cb.nranks_ = comm->nranks;
  decomposed = true;
}

void RankExchange::unique_id(void *id_out) {
  static_assert(sizeof(ncclUniqueId) == CONP_RCCL_ID_BYTES, "ncclUniqueId size");
  g_rccl.load();
  ncclUniqueId id;
  g_rccl.ok(g_rccl.GetUniqueId(&id), "ncclGetUniqueId");
  std::memcpy(id_out, &id, sizeof(id));
}

bool RankExchange::available() {
  try { g_rccl.load(); return true; } catch (...) { return false; }
}

void RankExchange::init_rccl(const void *id_in, int nranks, int rank) {
  if (comm) throw ConpError(CONP_ERR_STATE, "RCCL communicator already initialised");
  g_rccl.load();
  ncclUniqueId id;
  std::memcpy(&id, id_in, sizeof(id));
  g_rccl.ok(g_rccl.CommInitRank(&comm, nranks, id, rank), "ncclCommInitRank");
  comm_rank = rank;
}

void RankExchange::destroy_rccl() {
  if (comm) { (void)hipStreamSynchronize(ctx.stream); (void)g_rccl.CommDestroy(comm); comm = nullptr; }
}

void RankExchange::sum(double *d, size_t n, double *stage, const char *what) {
  if (comm) { g_rccl.ok(g_rccl.AllReduce(d, d, n, ncclDouble, ncclSum, comm, ctx.stream), what); return; }
  if (!cb.active())
    throw ConpError(CONP_ERR_STATE, "an update on several ranks needs conp_fix_comm_init_rccl or conp_fix_set_comm (or do the "
                                    "two collectives yourself between conp_fix_b_cal_device / _solve_device / _scatter_device)");
  HIP_TRY(hipMemcpyAsync(stage, d, n * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  ctx.sync();
  cb.sum(stage, (int64_t)n);
  HIP_TRY(hipMemcpyAsync(d, stage, n * sizeof(double), hipMemcpyHostToDevice, ctx.stream));
}

void RankExchange::gather_rows(double *d_full, int ne, int rows_per, int width, double *stage, const char *what) {
  const size_t w = (size_t)width;
  if (comm) {
    g_rccl.ok(g_rccl.AllGather(d_full + (size_t)comm_rank * rows_per * w, d_full, (size_t)rows_per * w, ncclDouble, comm, ctx.stream), what);
    return;
  }
  if (!cb.active()) return;
  std::vector<int> rows(cb.nranks_);
  for (int r = 0; r < cb.nranks_; ++r) rows[r] = std::min(ne, (r + 1) * rows_per) - std::min(ne, r * rows_per);
  const size_t row0 = (size_t)std::min(ne, cb.rank_ * rows_per), nr = (size_t)rows[cb.rank_];
  double *mine = stage + (size_t)ne * w;
  if (nr) HIP_TRY(hipMemcpyAsync(mine, d_full + row0 * w, nr * w * sizeof(double), hipMemcpyDeviceToHost, ctx.stream));
  ctx.sync();
  cb.gatherv(mine, rows, width, stage);
  HIP_TRY(hipMemcpyAsync(d_full, stage, (size_t)ne * w * sizeof(double), hipMemcpyHostToDevice, ctx.stream));
}

}  // namespace conp
