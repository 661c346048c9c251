#pragma once
// Which slot of a leased pool (device_mem.hpp: SlotPool) a call gets: pure functions of the slots as {dev, bytes, busy}, no HIP, so that the host
// compiler alone builds and tests them (tests/cpp/test_pool_pick_host.cpp).  Every rule looks at the idle slots of the caller's device only,
// breaks ties by the lower index, and answers with an index into the views or POOL_NEW_SLOT, and with the slots whose buffers are to be dropped.
#include <cstddef>
#include <vector>

namespace zk {

struct SlotView {
  int dev;
  size_t bytes;  // what the rule compares (the pool's own record of it, kept under its lock); 0: the slot holds no buffer
  bool busy;
};
constexpr int POOL_NEW_SLOT = -1;
struct PoolPick {
  int slot = POOL_NEW_SLOT;
  std::vector<int> drop;  // idle slots whose buffers go back to the device (the small workspaces' cap); may name `slot` itself
};

// DeviceBufPool: the smallest idle buffer that fits, else the largest idle one (its owner regrows it)
inline PoolPick pick_fit_else_largest(const std::vector<SlotView>& s, int dev, size_t bytes) {
  PoolPick r;
  for (int i = 0; i < (int)s.size(); ++i) {
    if (s[i].busy || s[i].dev != dev) continue;
    if (r.slot == POOL_NEW_SLOT) { r.slot = i; continue; }
    const size_t have = s[r.slot].bytes;
    if (s[i].bytes >= bytes ? (have < bytes || s[i].bytes < have) : (have < bytes && s[i].bytes > have)) r.slot = i;
  }
  return r;
}

// the largest idle buffer: what a grow-only pool wants when its callers' sizes repeat
inline PoolPick pick_largest(const std::vector<SlotView>& s, int dev) {
  PoolPick r;
  for (int i = 0; i < (int)s.size(); ++i)
    if (!s[i].busy && s[i].dev == dev && (r.slot == POOL_NEW_SLOT || s[i].bytes > s[r.slot].bytes)) r.slot = i;
  return r;
}
inline PoolPick pick_pinned(const std::vector<SlotView>& s, int dev) { return pick_largest(s, dev); }  // bytes: the pinned buffer's
inline PoolPick pick_stage(const std::vector<SlotView>& s, int dev) { return pick_largest(s, dev); }   // bytes: the two staging buffers' together

// The small workspaces (buffers of one power-of-two class `cls`, never regrown): the smallest idle buffer of this device that holds `cls`.
// Else a slot to allocate into -- the first idle slot that is empty, of any device, or that this pass empties -- and what to give back first:
// walking the idle slots in order, every buffer of this device goes while the pool (ALL slots' bytes, busy ones included) plus `cls`
// exceeds `cap`.  Never a busy slot, never another device's buffer.
inline PoolPick pick_small_ws(const std::vector<SlotView>& s, int dev, size_t cls, size_t cap) {
  PoolPick r;
  size_t pool = 0;
  for (int i = 0; i < (int)s.size(); ++i) {
    pool += s[i].bytes;
    if (s[i].busy || s[i].dev != dev || s[i].bytes == 0 || s[i].bytes < cls) continue;
    if (r.slot == POOL_NEW_SLOT || s[i].bytes < s[r.slot].bytes) r.slot = i;
  }
  if (r.slot != POOL_NEW_SLOT) return r;
  for (int i = 0; i < (int)s.size(); ++i) {
    if (s[i].busy) continue;
    if (s[i].bytes != 0) {
      if (pool + cls <= cap || s[i].dev != dev) continue;
      r.drop.push_back(i);
      pool -= s[i].bytes;
    }
    if (r.slot == POOL_NEW_SLOT) r.slot = i;
  }
  return r;
}

}  // namespace zk
