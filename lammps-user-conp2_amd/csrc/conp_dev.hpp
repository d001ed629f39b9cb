// Device plumbing shared by every host source of the library: the error type of the C ABI, guarded device buffers, the per-kernel
// profiler, and DevCtx -- what a component needs of a handle (its stream, the wait on it, the profiler).
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/conp_hip.h"

namespace conp::dev {

std::string &last_error();      // the calling thread's conp_last_error() text; defined once, in conp_dev.cpp

struct ConpError : std::runtime_error {
  int code;
  ConpError(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};

#define HIP_TRY(expr)                                                                                     \
  do {                                                                                                    \
    hipError_t e_ = (expr);                                                                               \
    if (e_ != hipSuccess)                                                                                 \
      throw ::conp::dev::ConpError(CONP_ERR_NO_DEVICE, std::string("HIP error: ") + hipGetErrorString(e_) + " at " #expr); \
  } while (0)

// CONP_GUARD=1 (diagnostic; tests/test_gpu_guard.py): every device buffer of the library is allocated with a 4-KB zone of a
// known byte pattern before and after it, and conp_debug_check_guards() reads all zones back -- an out-of-range STORE of any kernel
// shows up as a damaged zone with the buffer's size, instead of as silent corruption of a neighbouring allocation or as an abort
// of the HIP runtime somewhere else (round 3 had one abort whose message was lost).  Off: no cost.
struct GuardZones {
  static constexpr size_t G = 4096;
  static constexpr int PATTERN = 0xA5;
  std::mutex m;
  std::map<const void *, size_t> live;       // raw allocation -> payload bytes
  static bool on() { static const bool v = getenv("CONP_GUARD") != nullptr; return v; }
  static GuardZones &get();                  // the one registry of the library; defined once, in conp_dev.cpp
  int bad_freed = 0;                         // damaged zones found when a buffer was released (checked then: the zones go with it)
  std::string what_freed;
  void add(const void *raw, size_t bytes) { std::lock_guard<std::mutex> l(m); live[raw] = bytes; }
  void drop(const void *raw) {
    std::lock_guard<std::mutex> l(m);
    auto it = live.find(raw);
    if (it == live.end()) return;
    (void)hipDeviceSynchronize();
    bad_freed += check_one(static_cast<const char *>(raw), it->second, what_freed, bad_freed);
    live.erase(it);
  }
  static int check_one(const char *raw, size_t bytes, std::string &what, int already) {
    std::vector<unsigned char> h(2 * G);
    if (hipMemcpy(h.data(), raw, G, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(h.data() + G, raw + G + bytes, G, hipMemcpyDeviceToHost) != hipSuccess) { what += " [unreadable zone]"; return 1; }
    int bad = 0;
    for (int side = 0; side < 2; ++side) {
      size_t first = G;
      for (size_t i = 0; i < G; ++i) if (h[side * G + i] != PATTERN) { first = i; break; }
      if (first == G) continue;
      ++bad;
      if (already + bad <= 4) {
        char line[160];
        std::snprintf(line, sizeof line, " [buffer of %zu bytes: zone %s it damaged from byte %zu]", bytes, side ? "behind" : "before", first);
        what += line;
      }
    }
    return bad;
  }
  // number of damaged zones, of live buffers and of buffers released since the process started; `what` names the first few
  int check(std::string &what) {
    std::lock_guard<std::mutex> l(m);
    (void)hipDeviceSynchronize();
    int bad = bad_freed;
    what = what_freed;
    for (const auto &kv : live) bad += check_one(static_cast<const char *>(kv.first), kv.second, what, bad);
    return bad;
  }
};

template <typename T>
struct DevBuf {
  T *p = nullptr;
  size_t n = 0;
  void free_() {
    if (!p) return;
    if (GuardZones::on()) {
      char *raw = reinterpret_cast<char *>(p) - GuardZones::G;
      GuardZones::get().drop(raw);
      (void)hipFree(raw);
    } else (void)hipFree(p);
    p = nullptr;
  }
  ~DevBuf() { free_(); }
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  void reserve(size_t count) {
    if (count <= n) return;
    free_();
    const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
    if (GuardZones::on()) {
      constexpr size_t G = GuardZones::G;
      const size_t padded = (bytes + 15) / 16 * 16;
      char *raw = nullptr;
      HIP_TRY(hipMalloc(reinterpret_cast<void **>(&raw), padded + 2 * G));
      HIP_TRY(hipMemset(raw, GuardZones::PATTERN, G));
      HIP_TRY(hipMemset(raw + G + padded, GuardZones::PATTERN, G));
      GuardZones::get().add(raw, padded);
      p = reinterpret_cast<T *>(raw + G);
    } else HIP_TRY(hipMalloc(reinterpret_cast<void **>(&p), bytes));
    n = count;
  }
  void upload(const T *h, size_t count, hipStream_t s) {
    reserve(count);
    if (count) HIP_TRY(hipMemcpyAsync(p, h, count * sizeof(T), hipMemcpyHostToDevice, s));
  }
  void upload(const std::vector<T> &v, hipStream_t s) { upload(v.data(), v.size(), s); }
  void zero(hipStream_t s) { if (n) HIP_TRY(hipMemsetAsync(p, 0, n * sizeof(T), s)); }
  void release() { free_(); n = 0; }
};

// per-kernel timing with HIP events on the library's stream (bench.py's roofline leg)
struct Profiler {
  bool on = false;
  bool dominant_only = false;      // mode 2: events around sk_gemm only (cheap enough to ride inside a timed region)
  bool skipped = false;            // the begin() that belongs to the next end() recorded nothing
  unsigned n_dominant = 0;
  struct Rec { std::string name; hipEvent_t a, b; };
  std::vector<Rec> pending;
  std::vector<hipEvent_t> pool;    // events are reused: creating a pair per kernel per update costs host time
  std::vector<std::string> order;
  std::map<std::string, std::pair<double, int>> acc;
  std::vector<std::string> names_keep;
  hipEvent_t get() {
    hipEvent_t e = nullptr;
    if (!pool.empty()) { e = pool.back(); pool.pop_back(); }
    else (void)hipEventCreate(&e);
    return e;
  }
  void begin(const char *name, hipStream_t s) {
    if (!on) return;
    skipped = dominant_only && std::strcmp(name, "sk_gemm") != 0 && std::strcmp(name, "zn_gemm") != 0;
    // (an event pair drains the queue on both sides of the kernel: ~5 us per update when every launch carries one, measured
    //  0.3057 -> 0.3110 ms at the headline size; every 4th launch keeps the timed region within 0.4 % of an uninstrumented run)
    if (!skipped && dominant_only && (n_dominant++ & 3) != 0) skipped = true;
    if (skipped) return;
    if (pending.size() >= 4096) collect();        // a host that leaves profiling on for a long run must not grow this forever
    Rec r; r.name = name;
    r.a = get(); r.b = get();
    (void)hipEventRecord(r.a, s);
    pending.push_back(r);
  }
  void end(hipStream_t s) { if (on && !skipped && !pending.empty()) (void)hipEventRecord(pending.back().b, s); }
  void collect() {
    for (auto &r : pending) {
      (void)hipEventSynchronize(r.b);
      float ms = 0; (void)hipEventElapsedTime(&ms, r.a, r.b);
      if (!acc.count(r.name)) order.push_back(r.name);
      auto &e = acc[r.name]; e.first += ms; e.second += 1;
      pool.push_back(r.a); pool.push_back(r.b);
    }
    pending.clear();
  }
  void reset() { collect(); acc.clear(); order.clear(); n_dominant = 0; }
  ~Profiler() { for (auto e : pool) (void)hipEventDestroy(e); }
};

// what a component uses of a handle (conp_fix derives from it: conp_fix_set_stream reaches every holder of a DevCtx &)
struct DevCtx {
  hipStream_t stream = nullptr;
  Profiler prof;
  static double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }
  // The wait at the end of a host-buffer update: the runtime's blocking synchronisation wakes the thread tens of microseconds after
  // the stream drained; polling the stream for the first two milliseconds (an update takes 0.03 - 20 ms) returns within a few.
  // Longer waits (setup, large systems) fall back to the blocking call: no core is burnt for them.
  void sync() {
    const double t0 = now_s();
    for (;;) {
      const hipError_t e = hipStreamQuery(stream);
      if (e == hipSuccess) return;
      if (e != hipErrorNotReady) HIP_TRY(e);
      if (now_s() - t0 > 2e-3) break;
    }
    HIP_TRY(hipStreamSynchronize(stream));
  }
};

}  // namespace conp::dev
