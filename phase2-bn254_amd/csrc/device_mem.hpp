#pragma once
// The one place that allocates and frees device and pinned memory (the caches with their own accounting apart: the NTT table sets, the bases
// cache, mi355zk_malloc).  Three shapes of ownership -- DevBuf / PinnedBuf: a grow-only allocation that its owner keeps between calls; DevTemp:
// one call's temporary, freed when the call returns; StreamScratch: a DevBuf per (device, stream), bounded per device -- and SlotPool, the
// skeleton of the pools that lease such buffers to one call at a time (their choice rules: pool_pick.hpp).  Host code only.
#include <hip/hip_runtime.h>

#include <cstddef>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "device_util.hpp"
#include "pool_pick.hpp"

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

struct PinnedBuf {  // the same in pinned host memory
  void* p = nullptr;
  size_t bytes = 0;
  int reserve(size_t want) {
    if (bytes >= want) return ZK_OK;
    release();
    ZK_HIP(hipHostMalloc(&p, want, hipHostMallocDefault));
    bytes = want;
    return ZK_OK;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    bytes = 0;
  }
};

// One call's device temporary: a plain allocation, freed on every exit.  hipFree waits for the device, so an error exit may leave work
// queued; an exit that hands results to the caller has synchronised their stream before.
struct DevTemp {
  void* p = nullptr;
  DevTemp() = default;
  DevTemp(const DevTemp&) = delete;
  DevTemp& operator=(const DevTemp&) = delete;
  ~DevTemp() { if (p) (void)hipFree(p); }
  int alloc(size_t bytes) {  // once: a second call would lose the first allocation
    if (p) return ZK_ERR_BAD_ARGS;
    ZK_HIP(hipMalloc(&p, bytes));
    return ZK_OK;
  }
  template <class T>
  T* as(size_t byte_offset = 0) const { return reinterpret_cast<T*>(static_cast<char*>(p) + byte_offset); }
};

struct Events {  // a call's events, destroyed with it
  std::vector<hipEvent_t> e;
  unsigned flags;
  explicit Events(size_t count, unsigned event_flags = hipEventDisableTiming) : e(count, nullptr), flags(event_flags) {}
  hipError_t create() {
    hipError_t rc = hipSuccess;
    for (size_t i = 0; i < e.size() && rc == hipSuccess; ++i) rc = hipEventCreateWithFlags(&e[i], flags);
    return rc;
  }
  ~Events() {
    for (hipEvent_t x : e)
      if (x) (void)hipEventDestroy(x);
  }
  hipEvent_t operator[](size_t i) const { return e[i]; }
};

// One scratch buffer per (device, stream): calls on one stream are ordered by the stream itself, calls on different streams must not share
// a buffer.  Bounded: a caller that makes a stream per call must not pin a buffer per stream for ever, so past STREAMS_MAX streams of a
// device all of that device's buffers are dropped once the device is idle.
// NO LOCKING OF ITS OWN.  The caller holds, from get() until its last launch that uses the buffer is enqueued, the mutex under which EVERY
// user of this instance enqueues: then nobody else can be enqueueing work that uses a buffer of this instance, and after hipDeviceSynchronize
// none of them is in use.  An instance per family of callers -- two families on one stream would regrow each other's buffer.
class StreamScratch {
 public:
  static constexpr size_t STREAMS_MAX = 16;
  // the buffer of (dev, st), at least `bytes` long; dev is the current device
  int get(int dev, hipStream_t st, size_t bytes, void** out) {
    const auto key = std::make_pair(dev, st);
    if (bufs_.find(key) == bufs_.end()) {
      size_t mine = 0;
      for (auto& kv : bufs_) mine += kv.first.first == dev ? 1 : 0;
      if (mine >= STREAMS_MAX) {
        ZK_HIP(hipDeviceSynchronize());
        for (auto it = bufs_.begin(); it != bufs_.end();) {
          if (it->first.first != dev) { ++it; continue; }
          it->second.release();
          it = bufs_.erase(it);
        }
      }
    }
    DevBuf& b = bufs_[key];
    if (b.p && b.bytes < bytes) ZK_HIP(hipStreamSynchronize(st));  // earlier launches on this stream may still use the old buffer
    if (int rc = b.reserve(bytes)) return rc;
    *out = b.p;
    return ZK_OK;
  }
  void release_all() {
    for (auto& kv : bufs_) {
      (void)hipSetDevice(kv.first.first);
      kv.second.release();
    }
    bufs_.clear();
  }

 private:
  std::map<std::pair<int, hipStream_t>, DevBuf> bufs_;
};

// The skeleton of a pool whose slots are leased to one call at a time: the lock, the slots (on the heap: a lease keeps its pointer while
// the list grows), who holds which.  A user derives its slot from PoolSlot, gives it `size_t pool_bytes() const` (what its rule compares),
// names its choice rule (pool_pick.hpp) and does its own work on the slot it got OUTSIDE the lock (regrow, allocate, create streams): the
// slot is its alone while busy.  `busy` and `pooled` change under the lock only; the rules see `pooled`, never the holder's own fields.
// (A slot busy across release_all keeps its old `pooled` until its lease ends: a sum over the pool counts too much and may drop a buffer early.)
struct PoolSlot {
  int dev = -1;
  bool busy = false;
  size_t pooled = 0;  // pool_bytes() as of the slot's last hand-back (a holder that must publish earlier writes it under the lock itself)
};
template <class Slot>
struct SlotPool {
  std::mutex mu;
  std::vector<Slot*> slots;
  std::vector<SlotView> views;  // acquire's own, kept between calls: nothing is allocated under the lock once the pool has its slots

  // Under the lock: rule(views) chooses; a new slot where it says so; the slot becomes `dev`'s and busy; detach(slot) for every slot the
  // rule drops (the caller frees what it detached, outside).
  template <class Rule, class Detach = void (*)(Slot&)>
  Slot* acquire(int dev, Rule&& rule, Detach&& detach = [](Slot&) {}) {
    std::lock_guard<std::mutex> lk(mu);
    views.clear();
    for (const Slot* s : slots) views.push_back(SlotView{s->dev, s->pooled, s->busy});
    const PoolPick pick = rule(views);
    for (int d : pick.drop) {
      detach(*slots[d]);
      slots[d]->pooled = 0;
    }
    if (pick.slot == POOL_NEW_SLOT) slots.push_back(new Slot());
    Slot* s = pick.slot == POOL_NEW_SLOT ? slots.back() : slots[pick.slot];
    s->dev = dev;
    s->busy = true;
    return s;
  }

  // What a call holds.  `idle` == false: work that uses the slot may still be queued on `st`, which is synchronised before the slot goes back.
  struct Lease {
    SlotPool* pool = nullptr;
    Slot* slot = nullptr;
    hipStream_t st = nullptr;
    bool idle = true;
    Lease() = default;
    Lease(const Lease&) = delete;
    Lease& operator=(const Lease&) = delete;
    void hold(SlotPool* from, Slot* s, hipStream_t stream, bool is_idle) { pool = from, slot = s, st = stream, idle = is_idle; }
    void release() {
      if (slot == nullptr) return;
      if (!idle) (void)hipStreamSynchronize(st);
      std::lock_guard<std::mutex> lk(pool->mu);
      slot->pooled = slot->pool_bytes();
      slot->busy = false;
      slot = nullptr;
    }
    ~Lease() { release(); }
  };

  // free_slot(slot) on the slot's device for every slot, busy or not (mi355zk_shutdown); the slots themselves stay
  template <class Free>
  void release_all(Free&& free_slot) {
    std::lock_guard<std::mutex> lk(mu);
    for (Slot* s : slots) {
      (void)hipSetDevice(s->dev);
      free_slot(*s);
      if (!s->busy) s->pooled = s->pool_bytes();
    }
  }
};

}  // namespace zk
