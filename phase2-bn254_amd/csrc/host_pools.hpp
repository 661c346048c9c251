// What a host-buffer entry point holds while it runs: grow-only device buffers leased from a pool and a stage (a copy and a compute stream),
// over the types of device_mem.hpp (which also has the call's events); the device set of mi355zk_init and the fan-out of a call over it.
// Shared by host_entry.hip, host_ops.hip and accumulator_stream.hip; the stage pool and the device set themselves are host_pools.hip's.
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstddef>
#include <cstdlib>
#include <exception>
#include <mutex>
#include <thread>
#include <vector>

#include "device_mem.hpp"
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

// the device buffers of the host-buffer entry points (a call's uploads and results; msm_dev_entry's copy of a density map): grow-only
// buffers, leased per call -- hipMalloc / hipFree per call would synchronise the whole device and with it every other thread's multiexp
struct DeviceBufPool {
  struct Buf : PoolSlot, DevBuf {
    size_t pool_bytes() const { return bytes; }
  };
  static SlotPool<Buf>& pool() { static SlotPool<Buf> p; return p; }
  struct Lease {
    int acquire(int dev, size_t bytes, hipStream_t stream) {
      Buf* b = pool().acquire(dev, [&](const std::vector<SlotView>& v) { return pick_fit_else_largest(v, dev, bytes); });
      held_.hold(&pool(), b, stream, false);  // given back behind a synchronisation of `stream` (idle already after a completed call: the result came back over it)
      return b->reserve(bytes);  // (idle: its last user's stream was synchronised before the release)
    }
    void* p() const { return held_.slot ? held_.slot->p : nullptr; }  // the leased buffer; null once released
    void release() { held_.release(); }

   private:
    SlotPool<Buf>::Lease held_;
  };
};

// two staging buffers for scalar chunks, a bases buffer for uncached calls, the two streams.  Leased from a pool for the duration
// of a call (callers come and go -- the prover queues its multiexps from short-lived threads -- and their buffers must not pile up)
struct HostStage : PoolSlot {
  DevBuf sc[2];   // the scalar chunks' staging buffers
  DevBuf bases;
  DevBuf raw;     // strided records: one bounded piece of the caller's raw records on its way to records_pack
  hipStream_t copy = nullptr, compute = nullptr;
  size_t pool_bytes() const { return sc[0].bytes + sc[1].bytes; }
};
SlotPool<HostStage>& stage_pool();  // host_pools.hip

// What a host-buffer call holds while it runs: a stage (its two streams) and, with bytes > 0, one buffer of the pool.  On every exit
// both streams are idle before the buffer and then the stage go back: every exit of msm_host_run has joined its copy thread and the
// compute stream is idle after the last result came back, but an error path may leave work queued, copies into the buffer included.
struct CallLease {
  HostStage* S = nullptr;
  void* buf = nullptr;
  int open(int dev, size_t bytes = 0) {
    // the idle stage of this device with the largest staging buffers; a new one gets its streams here, outside the pool's lock
    S = stage_pool().acquire(dev, [&](const std::vector<SlotView>& v) { return pick_stage(v, dev); });
    stage_.hold(&stage_pool(), S, nullptr, true);  // (idle: the destructor synchronises both streams itself)
    if (S->copy == nullptr) ZK_HIP(hipStreamCreateWithFlags(&S->copy, hipStreamNonBlocking));
    if (S->compute == nullptr) ZK_HIP(hipStreamCreateWithFlags(&S->compute, hipStreamNonBlocking));
    if (bytes == 0) return ZK_OK;
    const int rc = pooled_.acquire(dev, bytes, S->compute);
    if (rc == ZK_OK) buf = pooled_.p();
    return rc;
  }
  ~CallLease() {
    if (S == nullptr) return;
    if (S->compute) (void)hipStreamSynchronize(S->compute);
    if (S->copy) (void)hipStreamSynchronize(S->copy);
    pooled_.release();
    stage_.release();
  }

 private:
  DeviceBufPool::Lease pooled_;
  SlotPool<HostStage>::Lease stage_;
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
