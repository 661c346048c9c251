#pragma once
// Device workspaces and pinned host buffers of the multiexp (msm_host.hpp).  Per unit ON PURPOSE (an anonymous namespace, unlike
// msm_common.hpp / msm_plan.hpp / msm_partition.hpp, which msm_g1.hip and msm_g2.hip share): G1 and G2 calls keep separate device
// workspaces, mutexes and pin pools, so a G1 and a G2 multiexp on one device never wait for each other's workspace.
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <vector>

#include "device_util.hpp"

namespace zk {

namespace {

struct Workspace {
  void* p = nullptr;
  size_t bytes = 0;
  std::mutex mu;                    // serialises the MSM calls that share this device's workspace
};
// per device: a process may drive several GPUs (mi355zk_init with n_devices > 1 runs one cell of a multiexp per device, each from
// its own host thread), and calls on different devices must not wait for each other
std::mutex g_ws_reg_mu;             // guards the map only
std::map<int, Workspace*> g_ws;
Workspace& ws_of(int dev) {
  std::lock_guard<std::mutex> lk(g_ws_reg_mu);
  Workspace*& w = g_ws[dev];
  if (w == nullptr) w = new Workspace();
  return *w;
}

int ws_reserve(Workspace& w, size_t bytes, void** out) {  // under w.mu
  if (w.bytes < bytes) {
    if (w.p) ZK_HIP(hipFree(w.p));
    w.p = nullptr;
    w.bytes = 0;
    ZK_HIP(hipMalloc(&w.p, bytes));
    w.bytes = bytes;
  }
  *out = w.p;
  return 0;
}

// Calls whose workspace is small (<= WS_SMALL: up to ~2^21 points) do not share the device-wide workspace and its lock: each
// leases a buffer from a pool for its duration.  The prover queues eight multiexps from eight threads (prover.rs:250-298) -- the
// short ones (inputs, B_G1 ...) then run concurrently on their callers' streams instead of waiting behind the long ones.  (A pool
// rather than a buffer per thread: callers come and go -- a thread pool per proof -- and their buffers must not pile up.)
constexpr size_t WS_SMALL = (size_t)1 << 30;
struct SmallWs {
  int dev = -1;
  void* p = nullptr;
  size_t bytes = 0;
  bool busy = false;
};
std::mutex g_tws_mu;
std::vector<SmallWs*> g_tws;  // the pool: as many entries as there have been concurrent calls

// Pinned host buffers for the one copy that ends a multiexp (the window sums and the error words): into pageable memory the runtime
// stages each copy (~20 us apiece at this size, twice per call); leased per call from a pool like the workspaces, grow-only.
struct PinBuf {
  int dev = -1;              // the device that was current when the buffer was allocated (a process may drive several)
  void* p = nullptr;
  size_t bytes = 0;
  bool busy = false;
};
std::mutex g_pin_mu;
std::vector<PinBuf*> g_pin;
struct PinLease {
  PinBuf* b = nullptr;
  ~PinLease() {
    if (b == nullptr) return;
    std::lock_guard<std::mutex> lk(g_pin_mu);
    b->busy = false;
  }
};
int pin_acquire(int dev, size_t bytes, PinLease* lease) {
  PinBuf* pick = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (PinBuf* b : g_pin)
      if (!b->busy && b->dev == dev && (pick == nullptr || b->bytes > pick->bytes)) pick = b;
    if (pick == nullptr) {
      pick = new PinBuf();
      pick->dev = dev;
      g_pin.push_back(pick);
    }
    pick->busy = true;
  }
  lease->b = pick;
  if (pick->bytes < bytes) {
    if (pick->p) (void)hipHostFree(pick->p);
    pick->p = nullptr;
    pick->bytes = 0;
    size_t want = 65536;
    while (want < bytes) want <<= 1;
    ZK_HIP(hipHostMalloc(&pick->p, want, hipHostMallocDefault));
    pick->bytes = want;
  }
  return ZK_OK;
}
struct SmallWsLease {
  SmallWs* w = nullptr;
  hipStream_t st = nullptr;
  bool idle = false;  // set once the caller has synchronised the stream after its last use of the buffer
  ~SmallWsLease() {
    if (w == nullptr) return;
    if (!idle) (void)hipStreamSynchronize(st);  // an error path: kernels using the buffer may still be queued
    std::lock_guard<std::mutex> lk(g_tws_mu);
    w->busy = false;
  }
};
// Buffers come in power-of-two sizes (>= 16 MiB) and are never regrown: hipFree / hipMalloc synchronise the device, and eight
// concurrent calls of eight different sizes would otherwise keep trading buffers.  Idle buffers are only given back when the pool
// exceeds TWS_POOL_CAP.
constexpr size_t TWS_POOL_CAP = (size_t)12 << 30;
int tws_acquire(int dev, size_t bytes, hipStream_t st, SmallWsLease* lease, void** out) {
  size_t cls = (size_t)16 << 20;
  while (cls < bytes) cls <<= 1;
  SmallWs* pick = nullptr;
  std::vector<void*> drop;
  {
    std::lock_guard<std::mutex> lk(g_tws_mu);
    size_t pool = 0;
    for (SmallWs* w : g_tws) {  // the smallest idle buffer that fits
      pool += w->bytes;
      if (w->busy || w->dev != dev || w->p == nullptr || w->bytes < cls) continue;
      if (pick == nullptr || w->bytes < pick->bytes) pick = w;
    }
    if (pick == nullptr) {
      for (SmallWs* w : g_tws) {  // an empty slot, and room under the cap
        if (w->busy) continue;
        if (w->p == nullptr) { if (pick == nullptr) pick = w; continue; }
        if (pool + cls > TWS_POOL_CAP && w->dev == dev) {
          drop.push_back(w->p);
          pool -= w->bytes;
          w->p = nullptr;
          w->bytes = 0;
          if (pick == nullptr) pick = w;
        }
      }
      if (pick == nullptr) {
        pick = new SmallWs();
        g_tws.push_back(pick);
      }
      pick->dev = dev;
    }
    pick->busy = true;
  }
  lease->w = pick;
  lease->st = st;
  lease->idle = true;  // nothing queued on it yet
  for (void* d : drop) (void)hipFree(d);  // idle: their last users synchronised before releasing them
  void* p = pick->p;   // (ours: busy was set under the lock)
  if (p == nullptr) {
    ZK_HIP(hipMalloc(&p, cls));
    // published under the lock: another thread's scan sums `bytes` over ALL slots, busy ones included (r6: ThreadSanitizer on the GPU box
    // reported this write against that read, profiles/r06_tsan.txt -- the only report inside this library)
    std::lock_guard<std::mutex> lk(g_tws_mu);
    pick->p = p;
    pick->bytes = cls;
  }
  lease->idle = false;
  *out = p;
  return 0;
}

void ws_release_all() {
  {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (PinBuf* b : g_pin) {
      if (b->busy) continue;
      (void)hipSetDevice(b->dev);
      if (b->p) (void)hipHostFree(b->p);
      b->p = nullptr;
      b->bytes = 0;
    }
  }
  {
    std::lock_guard<std::mutex> lk(g_tws_mu);
    for (SmallWs* t : g_tws) {
      if (t->p) {
        (void)hipSetDevice(t->dev);
        (void)hipFree(t->p);
      }
      t->p = nullptr;
      t->bytes = 0;
    }
  }
  std::lock_guard<std::mutex> lk(g_ws_reg_mu);
  for (auto& kv : g_ws) {
    std::lock_guard<std::mutex> wl(kv.second->mu);
    (void)hipSetDevice(kv.first);
    (void)hipFree(kv.second->p);
    kv.second->p = nullptr;
    kv.second->bytes = 0;
  }
}

}  // namespace

}  // namespace zk
