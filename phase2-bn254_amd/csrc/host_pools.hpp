// What a host-buffer entry point holds while it runs: grow-only device buffers leased from a pool, a stage (a copy and a compute stream) and
// the call's events.  Shared by host_entry.hip (which owns the stage pool) and accumulator_stream.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <mutex>
#include <vector>

#include "device_util.hpp"

namespace zk {
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
extern std::mutex g_stage_mu;      // host_entry.hip: the pool of stages
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
}  // namespace zk
