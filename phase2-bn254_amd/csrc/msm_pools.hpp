#pragma once
// Device workspaces and pinned host buffers of the multiexp (msm_host.hpp).  Per unit ON PURPOSE (an anonymous namespace, unlike
// msm_common.hpp / msm_plan.hpp / msm_partition.hpp, which msm_g1.hip and msm_g2.hip share): G1 and G2 calls keep separate device
// workspaces, mutexes and pin pools, so a G1 and a G2 multiexp on one device never wait for each other's workspace.  Only the types
// (device_mem.hpp) are shared.
#include <hip/hip_runtime.h>

#include <map>
#include <mutex>
#include <vector>

#include "device_mem.hpp"
#include "device_util.hpp"

namespace zk {

namespace {

struct Workspace {
  DevBuf buf;                       // reserved under mu
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

// Pinned host buffers for the one copy that ends a multiexp (the window sums and the error words): into pageable memory the runtime
// stages each copy (~20 us apiece at this size, twice per call); leased per call from a pool like the workspaces, grow-only.
struct PinBuf : PoolSlot, PinnedBuf {  // dev: the device that was current when the buffer was allocated (a process may drive several)
  size_t pool_bytes() const { return bytes; }
};
SlotPool<PinBuf> g_pin;
using PinLease = SlotPool<PinBuf>::Lease;
int pin_acquire(int dev, size_t bytes, PinLease* lease) {
  PinBuf* pick = g_pin.acquire(dev, [&](const std::vector<SlotView>& v) { return pick_pinned(v, dev); });
  lease->hold(&g_pin, pick, nullptr, true);  // (the caller synchronises its stream before it reads the buffer)
  size_t want = 65536;
  while (want < bytes) want <<= 1;
  return pick->reserve(want);
}

// Calls whose workspace is small (<= WS_SMALL: up to ~2^21 points) do not share the device-wide workspace and its lock: each
// leases a buffer from a pool for its duration.  The prover queues eight multiexps from eight threads (prover.rs:250-298) -- the
// short ones (inputs, B_G1 ...) then run concurrently on their callers' streams instead of waiting behind the long ones.  (A pool
// rather than a buffer per thread: callers come and go -- a thread pool per proof -- and their buffers must not pile up.)
constexpr size_t WS_SMALL = (size_t)1 << 30;
struct SmallWs : PoolSlot {
  DevBuf buf;
  size_t pool_bytes() const { return buf.bytes; }
};
SlotPool<SmallWs> g_tws;  // as many slots as there have been concurrent calls
// idle: set once the caller has synchronised the stream after its last use of the buffer (else an error path: kernels using it may still be queued)
using SmallWsLease = SlotPool<SmallWs>::Lease;
// Buffers come in power-of-two sizes (>= 16 MiB) and are never regrown: hipFree / hipMalloc synchronise the device, and eight
// concurrent calls of eight different sizes would otherwise keep trading buffers.  Idle buffers are only given back when the pool
// exceeds TWS_POOL_CAP.
constexpr size_t TWS_POOL_CAP = (size_t)12 << 30;
int tws_acquire(int dev, size_t bytes, hipStream_t st, SmallWsLease* lease, void** out) {
  size_t cls = (size_t)16 << 20;
  while (cls < bytes) cls <<= 1;
  std::vector<DevBuf> drop;
  SmallWs* pick = g_tws.acquire(
      dev, [&](const std::vector<SlotView>& v) { return pick_small_ws(v, dev, cls, TWS_POOL_CAP); }, [&](SmallWs& w) { drop.push_back(w.buf); w.buf = DevBuf(); });
  lease->hold(&g_tws, pick, st, true);  // nothing queued on it yet
  for (DevBuf& d : drop) d.release();   // idle: their last users synchronised before releasing them
  void* p = pick->buf.p;                // (ours: busy was set under the lock)
  if (p == nullptr) {
    DevBuf fresh;
    if (int rc = fresh.reserve(cls)) return rc;
    p = fresh.p;
    // published under the lock: another thread's scan sums `bytes` over ALL slots, busy ones included (r6: ThreadSanitizer on the GPU box
    // reported this write against that read, profiles/r06_tsan.txt -- the only report inside this library)
    std::lock_guard<std::mutex> lk(g_tws.mu);
    pick->buf = fresh;
    pick->pooled = cls;
  }
  lease->idle = false;
  *out = p;
  return 0;
}

void ws_release_all() {
  g_pin.release_all([](PinBuf& b) { if (!b.busy) b.release(); });
  g_tws.release_all([](SmallWs& t) { t.buf.release(); });
  std::lock_guard<std::mutex> lk(g_ws_reg_mu);
  for (auto& kv : g_ws) {
    std::lock_guard<std::mutex> wl(kv.second->mu);
    (void)hipSetDevice(kv.first);
    kv.second->buf.release();
  }
}

}  // namespace

}  // namespace zk
