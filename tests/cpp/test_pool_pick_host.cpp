// The choice rules of the leased pools (phase2-bn254_amd/csrc/pool_pick.hpp) without a GPU: hand-written slot tables with the picks they
// must give, and 10 000 random tables per rule against a restatement of the loops the pools ran before the rules were pure functions.
// The restatements below are the EXPECTATION: written out here on purpose, sharing nothing with the header.
//   test_pool_pick_host            -> "ok <checks>" and exit code 0, or the failed checks on stderr and exit code 1
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

#include "../../phase2-bn254_amd/csrc/pool_pick.hpp"

using zk::POOL_NEW_SLOT;
using zk::PoolPick;
using zk::SlotView;
using Table = std::vector<SlotView>;
using Drop = std::vector<int>;

static int g_checks = 0, g_failed = 0;
static std::string show(const Drop& d) {
  std::string s = "{";
  for (int i : d) s += std::to_string(i) + ",";
  return s + "}";
}
static void expect(const char* what, const PoolPick& got, int slot, const Drop& drop = {}) {
  ++g_checks;
  if (got.slot == slot && got.drop == drop) return;
  ++g_failed;
  std::fprintf(stderr, "FAILED %s: slot %d drop %s, expected slot %d drop %s\n", what, got.slot, show(got.drop).c_str(), slot, show(drop).c_str());
}

// ---- the loops as the pools ran them, over records with a pointer like theirs
struct OldSlot {
  int dev;
  size_t bytes;
  bool busy;
  bool has_p;  // p != nullptr
};
static std::vector<OldSlot> old_of(const Table& t) {
  std::vector<OldSlot> o;
  for (const SlotView& s : t) o.push_back(OldSlot{s.dev, s.bytes, s.busy, s.bytes != 0});
  return o;
}
static int index_of(const std::vector<OldSlot>& all, const OldSlot* x) { return x ? (int)(x - all.data()) : POOL_NEW_SLOT; }

static PoolPick old_device_buf_pool(const Table& t, int dev, size_t bytes) {
  const std::vector<OldSlot> all = old_of(t);
  const OldSlot* b = nullptr;
  for (const OldSlot& x : all)
    if (!x.busy && x.dev == dev) {
      if (b == nullptr) { b = &x; continue; }
      const bool fits = x.bytes >= bytes, bfits = b->bytes >= bytes;
      if (fits ? (!bfits || x.bytes < b->bytes) : (!bfits && x.bytes > b->bytes)) b = &x;
    }
  PoolPick r;
  r.slot = index_of(all, b);
  return r;
}
static PoolPick old_pin_acquire(const Table& t, int dev) {
  const std::vector<OldSlot> all = old_of(t);
  const OldSlot* pick = nullptr;
  for (const OldSlot& b : all)
    if (!b.busy && b.dev == dev && (pick == nullptr || b.bytes > pick->bytes)) pick = &b;
  PoolPick r;
  r.slot = index_of(all, pick);
  return r;
}
static PoolPick old_host_stage(const Table& t, int dev) {  // bytes: sc[0].bytes + sc[1].bytes
  const std::vector<OldSlot> all = old_of(t);
  const OldSlot* mine = nullptr;
  for (const OldSlot& s : all)
    if (!s.busy && s.dev == dev && (mine == nullptr || s.bytes > mine->bytes)) mine = &s;
  PoolPick r;
  r.slot = index_of(all, mine);
  return r;
}
static PoolPick old_tws_acquire(const Table& t, int dev, size_t cls, size_t cap) {
  std::vector<OldSlot> all = old_of(t);
  OldSlot* pick = nullptr;
  PoolPick r;
  size_t pool = 0;
  for (OldSlot& w : all) {  // the smallest idle buffer that fits
    pool += w.bytes;
    if (w.busy || w.dev != dev || !w.has_p || w.bytes < cls) continue;
    if (pick == nullptr || w.bytes < pick->bytes) pick = &w;
  }
  if (pick == nullptr) {
    for (OldSlot& w : all) {  // an empty slot, and room under the cap
      if (w.busy) continue;
      if (!w.has_p) { if (pick == nullptr) pick = &w; continue; }
      if (pool + cls > cap && w.dev == dev) {
        r.drop.push_back((int)(&w - all.data()));
        pool -= w.bytes;
        w.has_p = false;
        w.bytes = 0;
        if (pick == nullptr) pick = &w;
      }
    }
  }
  r.slot = index_of(all, pick);
  return r;
}

// ---- hand-written tables
static const bool BUSY = true, IDLE = false;

static void fixed_device_buf_pool() {
  using zk::pick_fit_else_largest;
  expect("buf empty pool", pick_fit_else_largest({}, 0, 100), POOL_NEW_SLOT);
  expect("buf all busy", pick_fit_else_largest({{0, 500, BUSY}, {0, 50, BUSY}}, 0, 100), POOL_NEW_SLOT);
  expect("buf other device", pick_fit_else_largest({{1, 500, IDLE}, {2, 100, IDLE}}, 0, 100), POOL_NEW_SLOT);
  expect("buf other device beside ours", pick_fit_else_largest({{1, 100, IDLE}, {0, 10, IDLE}}, 0, 100), 1);
  expect("buf exact fit before a larger fit", pick_fit_else_largest({{0, 400, IDLE}, {0, 100, IDLE}, {0, 200, IDLE}}, 0, 100), 1);
  expect("buf smallest fit, not the first", pick_fit_else_largest({{0, 400, IDLE}, {0, 50, IDLE}, {0, 200, IDLE}}, 0, 100), 2);
  expect("buf a fit replaces a misfit", pick_fit_else_largest({{0, 50, IDLE}, {0, 400, IDLE}}, 0, 100), 1);
  expect("buf a misfit never replaces a fit", pick_fit_else_largest({{0, 400, IDLE}, {0, 50, IDLE}, {0, 99, IDLE}}, 0, 100), 0);
  expect("buf nothing fits: the largest", pick_fit_else_largest({{0, 10, IDLE}, {0, 90, IDLE}, {0, 50, IDLE}, {0, 900, BUSY}}, 0, 100), 1);
  expect("buf tie of fits: the first", pick_fit_else_largest({{0, 200, IDLE}, {0, 200, IDLE}}, 0, 100), 0);
  expect("buf tie of misfits: the first", pick_fit_else_largest({{0, 0, IDLE}, {0, 0, IDLE}}, 0, 100), 0);
  expect("buf busy fit skipped", pick_fit_else_largest({{0, 100, BUSY}, {0, 300, IDLE}}, 0, 100), 1);
  expect("buf zero bytes fits anything", pick_fit_else_largest({{0, 64, IDLE}, {0, 0, IDLE}}, 0, 0), 1);
}

static void fixed_largest(const char* name, PoolPick (*rule)(const Table&, int)) {
  const std::string n(name);
  expect((n + " empty pool").c_str(), rule({}, 0), POOL_NEW_SLOT);
  expect((n + " all busy").c_str(), rule({{0, 500, BUSY}, {0, 50, BUSY}}, 0), POOL_NEW_SLOT);
  expect((n + " other device").c_str(), rule({{1, 500, IDLE}}, 0), POOL_NEW_SLOT);
  expect((n + " other device larger").c_str(), rule({{1, 500, IDLE}, {0, 5, IDLE}}, 0), 1);
  expect((n + " largest").c_str(), rule({{0, 100, IDLE}, {0, 300, IDLE}, {0, 200, IDLE}}, 0), 1);
  expect((n + " largest is busy").c_str(), rule({{0, 100, IDLE}, {0, 300, BUSY}, {0, 200, IDLE}}, 0), 2);
  expect((n + " tie: the first").c_str(), rule({{0, 300, IDLE}, {0, 300, IDLE}}, 0), 0);
  expect((n + " empty slots: the first").c_str(), rule({{1, 0, IDLE}, {0, 0, IDLE}, {0, 0, IDLE}}, 0), 1);
}

static void fixed_small_ws() {
  using zk::pick_small_ws;
  const size_t CAP = 1000;
  expect("ws empty pool", pick_small_ws({}, 0, 16, CAP), POOL_NEW_SLOT);
  expect("ws all busy", pick_small_ws({{0, 16, BUSY}, {0, 64, BUSY}}, 0, 16, CAP), POOL_NEW_SLOT);
  expect("ws other device's buffer, room under the cap", pick_small_ws({{1, 16, IDLE}}, 0, 16, CAP), POOL_NEW_SLOT);
  expect("ws exact fit before a larger fit", pick_small_ws({{0, 64, IDLE}, {0, 16, IDLE}, {0, 32, IDLE}}, 0, 16, CAP), 1);
  expect("ws smallest fit", pick_small_ws({{0, 64, IDLE}, {0, 8, IDLE}, {0, 32, IDLE}}, 0, 16, CAP), 2);
  expect("ws tie: the first", pick_small_ws({{0, 32, IDLE}, {0, 32, IDLE}}, 0, 16, CAP), 0);
  expect("ws busy fit skipped", pick_small_ws({{0, 16, BUSY}, {0, 64, IDLE}}, 0, 16, CAP), 1);
  expect("ws nothing fits, room: a new slot", pick_small_ws({{0, 8, IDLE}, {0, 4, BUSY}}, 0, 16, CAP), POOL_NEW_SLOT);
  expect("ws nothing fits: the empty slot", pick_small_ws({{0, 8, IDLE}, {0, 0, IDLE}}, 0, 16, CAP), 1);
  expect("ws an empty slot of another device serves", pick_small_ws({{1, 0, IDLE}, {0, 0, IDLE}}, 0, 16, CAP), 0);
  expect("ws a busy empty slot (being allocated) does not", pick_small_ws({{0, 0, BUSY}}, 0, 16, CAP), POOL_NEW_SLOT);
  // the cap: pool + class just under, at and over it
  expect("ws pool + class under the cap", pick_small_ws({{0, 8, IDLE}, {0, 975, BUSY}}, 0, 16, CAP), POOL_NEW_SLOT);
  expect("ws pool + class at the cap", pick_small_ws({{0, 8, IDLE}, {0, 976, BUSY}}, 0, 16, CAP), POOL_NEW_SLOT);
  expect("ws pool + class over the cap", pick_small_ws({{0, 8, IDLE}, {0, 977, BUSY}}, 0, 16, CAP), 0, {0});
  expect("ws drops stop once under the cap", pick_small_ws({{0, 8, IDLE}, {0, 8, IDLE}, {0, 8, IDLE}, {0, 970, BUSY}}, 0, 16, CAP), 0, {0, 1});
  expect("ws drops only this device's", pick_small_ws({{1, 8, IDLE}, {0, 8, IDLE}, {0, 990, BUSY}}, 0, 16, CAP), 1, {1});
  expect("ws never drops a busy one", pick_small_ws({{0, 8, BUSY}, {0, 990, BUSY}}, 0, 16, CAP), POOL_NEW_SLOT);
  expect("ws nothing of this device to drop", pick_small_ws({{1, 8, IDLE}, {2, 990, IDLE}}, 0, 16, CAP), POOL_NEW_SLOT);
  expect("ws the empty slot before it stays the pick", pick_small_ws({{0, 0, IDLE}, {0, 8, IDLE}, {0, 990, BUSY}}, 0, 16, CAP), 0, {1});
  expect("ws the empty slot behind a dropped one does not", pick_small_ws({{0, 8, IDLE}, {0, 0, IDLE}, {0, 990, BUSY}}, 0, 16, CAP), 0, {0});
  expect("ws a fit is taken whatever the cap says", pick_small_ws({{0, 8, IDLE}, {0, 16, IDLE}, {0, 990, BUSY}}, 0, 16, CAP), 1);
}

// ---- random tables
static uint64_t g_rng = 0x243f6a8885a308d3ull;
static uint32_t rnd(uint32_t below) {
  g_rng ^= g_rng << 13, g_rng ^= g_rng >> 7, g_rng ^= g_rng << 17;
  return (uint32_t)((g_rng >> 20) % below);
}
static bool same(const PoolPick& a, const PoolPick& b) { return a.slot == b.slot && a.drop == b.drop; }
static void report_random(const char* rule, const Table& t, int dev, size_t arg, const PoolPick& got, const PoolPick& want) {
  ++g_failed;
  std::fprintf(stderr, "FAILED random %s dev %d arg %zu:", rule, dev, arg);
  for (const SlotView& s : t) std::fprintf(stderr, " (%d,%zu,%d)", s.dev, s.bytes, (int)s.busy);
  std::fprintf(stderr, " -> slot %d drop %s, the old loop: slot %d drop %s\n", got.slot, show(got.drop).c_str(), want.slot, show(want.drop).c_str());
}
static void random_tables() {
  static const size_t SIZES[] = {0, 0, 16, 16, 32, 32, 64, 128, 24, 200};  // classes, repeats (ties), empty slots, a size that is no class
  for (int it = 0; it < 10000; ++it) {
    Table t(rnd(13));  // 0 .. 12 slots
    for (SlotView& s : t) s = SlotView{(int)rnd(3), SIZES[rnd(10)], rnd(3) == 0};
    const int dev = (int)rnd(3);
    const size_t want = SIZES[2 + rnd(8)], cls = (size_t)16 << rnd(3), cap = 64 + rnd(400);
    PoolPick a = zk::pick_fit_else_largest(t, dev, want), b = old_device_buf_pool(t, dev, want);
    if (!same(a, b)) report_random("device buffers", t, dev, want, a, b);
    a = zk::pick_pinned(t, dev), b = old_pin_acquire(t, dev);
    if (!same(a, b)) report_random("pinned", t, dev, 0, a, b);
    a = zk::pick_stage(t, dev), b = old_host_stage(t, dev);
    if (!same(a, b)) report_random("stage", t, dev, 0, a, b);
    a = zk::pick_small_ws(t, dev, cls, cap), b = old_tws_acquire(t, dev, cls, cap);
    if (!same(a, b)) report_random("small workspace", t, dev, cls * 1000 + cap, a, b);
    g_checks += 4;
  }
}

int main() {
  fixed_device_buf_pool();
  fixed_largest("pinned", zk::pick_pinned);
  fixed_largest("stage", zk::pick_stage);
  fixed_small_ws();
  random_tables();
  if (g_failed) {
    std::fprintf(stderr, "%d of %d checks failed\n", g_failed, g_checks);
    return 1;
  }
  std::printf("ok %d\n", g_checks);
  return 0;
}
