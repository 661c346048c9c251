// What a host-buffer entry point holds while it runs: grow-only device buffers leased from a pool, a stage (a copy and a compute stream) and
// the call's events; the device set of mi355zk_init and the fan-out of a call over it.  Shared by host_entry.hip, host_ops.hip and
// accumulator_stream.hip; the stage pool and the device set themselves are host_pools.hip's.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstddef>
#include <cstdlib>
#include <exception>
#include <mutex>
#include <thread>
#include <vector>

#include "device_util.hpp"

namespace zk {
struct DeviceGuard {  // the calling thread's current device is its own business: restore it
  int prev = -1;
  DeviceGuard() { if (hipGetDevice(&prev) != hipSuccess) prev = -1; }
  ~DeviceGuard() { if (prev >= 0) (void)hipSetDevice(prev); }
};

inline bool trace_host() {  // MI355ZK_TRACE_HOST: timeline of the streamed / multi-device call on stderr
  static const bool on = std::getenv("MI355ZK_TRACE_HOST") != nullptr;
  return on;
}
inline double ms_since(std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); }

// a grow-only device allocation.  reserve() regrows by free + malloc: the owner knows that nothing queued still uses the old one
struct DevBuf {
  void* p = nullptr;
  size_t bytes = 0;
  int reserve(size_t want) {
    if (bytes >= want) return ZK_OK;
    if (p) ZK_HIP(hipFree(p));
    p = nullptr;
    bytes = 0;
    ZK_HIP(hipMalloc(&p, want));
    bytes = want;
    return ZK_OK;
  }
  void release() {  // (on the current device)
    (void)hipFree(p);
    p = nullptr;
    bytes = 0;
  }
};

// the device buffers of the host-buffer entry points (a call's uploads and results; msm_dev_entry's copy of a density map): grow-only
// buffers, leased per call -- hipMalloc / hipFree per call would synchronise the whole device and with it every other thread's multiexp
struct DeviceBufPool {
  struct Buf : DevBuf {
    int dev = -1;
    bool busy = false;
  };
  static std::mutex& mu() { static std::mutex m; return m; }
  static std::vector<Buf*>& all() { static std::vector<Buf*> v; return v; }
  struct Lease {
    Buf* b = nullptr;
    hipStream_t st = nullptr;
    int acquire(int dev, size_t bytes, hipStream_t stream) {
      st = stream;
      {
        std::lock_guard<std::mutex> lk(mu());
        for (Buf* x : all())  // the smallest idle buffer that fits, else the largest idle one (regrown below)
          if (!x->busy && x->dev == dev) {
            if (b == nullptr) { b = x; continue; }
            const bool fits = x->bytes >= bytes, bfits = b->bytes >= bytes;
            if (fits ? (!bfits || x->bytes < b->bytes) : (!bfits && x->bytes > b->bytes)) b = x;
          }
        if (b == nullptr) {
          b = new Buf();
          b->dev = dev;
          all().push_back(b);
        }
        b->busy = true;
      }
      return b->reserve(bytes);  // (idle: its last user's stream was synchronised before the release)
    }
    void release() {
      if (b == nullptr) return;
      (void)hipStreamSynchronize(st);  // (idle already after a completed call: the result came back over this stream)
      std::lock_guard<std::mutex> lk(mu());
      b->busy = false;
      b = nullptr;
    }
    ~Lease() { release(); }
  };
};

// two staging buffers for scalar chunks, a bases buffer for uncached calls, the two streams.  Leased from a pool for the duration
// of a call (callers come and go -- the prover queues its multiexps from short-lived threads -- and their buffers must not pile up)
struct HostStage {
  int dev = -1;
  bool busy = false;
  DevBuf sc[2];   // the scalar chunks' staging buffers
  DevBuf bases;
  DevBuf raw;     // strided records: one bounded piece of the caller's raw records on its way to records_pack
  hipStream_t copy = nullptr, compute = nullptr;
};
extern std::mutex g_stage_mu;      // host_pools.hip: the pool of stages
HostStage* host_stage(int dev);    // an idle stage of the device, marked busy (nullptr: no streams to be had)

// What a host-buffer call holds while it runs: a stage (its two streams) and, with bytes > 0, one buffer of the pool.  On every exit
// both streams are idle before the buffer and then the stage go back: every exit of msm_host_run has joined its copy thread and the
// compute stream is idle after the last result came back, but an error path may leave work queued, copies into the buffer included.
struct CallLease {
  HostStage* S = nullptr;
  void* buf = nullptr;
  int open(int dev, size_t bytes = 0) {
    S = host_stage(dev);
    if (S == nullptr) return ZK_ERR_DEVICE;
    if (bytes == 0) return ZK_OK;
    const int rc = pooled_.acquire(dev, bytes, S->compute);
    if (rc == ZK_OK) buf = pooled_.b->p;
    return rc;
  }
  ~CallLease() {
    if (S == nullptr) return;
    (void)hipStreamSynchronize(S->compute);
    (void)hipStreamSynchronize(S->copy);
    pooled_.release();
    std::lock_guard<std::mutex> lk(g_stage_mu);
    S->busy = false;
  }

 private:
  DeviceBufPool::Lease pooled_;
};

// a call's events (no timing), destroyed with it
struct Events {
  std::vector<hipEvent_t> e;
  explicit Events(size_t count) : e(count, nullptr) {}
  hipError_t create() {
    hipError_t rc = hipSuccess;
    for (size_t i = 0; i < e.size() && rc == hipSuccess; ++i) rc = hipEventCreateWithFlags(&e[i], hipEventDisableTiming);
    return rc;
  }
  ~Events() {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
  hipEvent_t operator[](size_t i) const { return e[i]; }
};

// The device set of mi355zk_init (host_pools.hip): HIP device ids; a test may repeat one id (logical devices sharing a GPU).
void devset_set(const std::vector<int>& set);   // (empty: the current device)
int devset_count();
std::vector<int> devset_snapshot();
int devset_or_current(std::vector<int>* devs);  // the device set, or the calling thread's current device when none was given
unsigned devset_turn();                         // a counter that deals short calls out to the devices of the set in turn
void host_entry_release_all();                  // the device memory of the bases cache, the stages and the buffer pool (mi355zk_shutdown)

// The fan-out of a call over its cells / ranges / workers: fn(0) .. fn(count - 1), unit 0 on the calling thread, every other unit on a host
// thread of its own; the units whose thread could not be had run here afterwards, one after the other.  Returns the units' return codes.
// Nothing is thrown out of a host thread or across the C ABI (std::bad_alloc from a staging vector, a std::system_error from a lock): the
// unit fails as a device error.  The calling thread's current device is restored.
template <class Fn>
std::vector<int> fan_out(size_t count, Fn&& fn) {
  std::vector<int> rcs(count, ZK_OK);
  auto unit = [&](size_t i) noexcept {
    try {
      rcs[i] = fn(i);
    } catch (...) {
      rcs[i] = ZK_ERR_DEVICE;
    }
  };
  DeviceGuard guard;
  std::vector<std::thread> th;
  size_t started = 1;
  try {
    for (; started < count; ++started) th.emplace_back([&, started] { unit(started); });
  } catch (const std::exception&) {
    // (no more host threads to be had -- nothing is thrown across the C ABI)
  }
  if (count) unit(0);
  for (size_t i = started; i < count; ++i) unit(i);
  for (auto& t : th) t.join();
  return rcs;
}
inline int first_error(const std::vector<int>& rcs) {
  for (int rc : rcs)
    if (rc != ZK_OK) return rc;
  return ZK_OK;
}
}  // namespace zk
