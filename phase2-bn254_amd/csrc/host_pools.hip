// The state behind host_pools.hpp: the pool of stages, the device set of mi355zk_init, and the release of everything the host-buffer entry
// points keep on the devices.  Host code only.
#include "host_pools.hpp"

#include <atomic>

#include "bases_cache.hpp"

namespace zk {
SlotPool<HostStage>& stage_pool() {  // as many stages as there have been concurrent host-buffer calls (CallLease::open leases them)
  static SlotPool<HostStage> pool;
  return pool;
}

static std::mutex g_devset_mu;
static std::vector<int> g_devset;                 // HIP device ids of the set (a test may repeat one id: logical devices sharing a GPU)
static std::atomic<unsigned> g_devset_turn{0};

void devset_set(const std::vector<int>& set) {
  std::lock_guard<std::mutex> lk(g_devset_mu);
  g_devset = set;
}
int devset_count() {
  std::lock_guard<std::mutex> lk(g_devset_mu);
  return g_devset.empty() ? 1 : (int)g_devset.size();
}
std::vector<int> devset_snapshot() {
  std::lock_guard<std::mutex> lk(g_devset_mu);
  return g_devset;
}
int devset_or_current(std::vector<int>* devs) {
  *devs = devset_snapshot();
  if (devs->empty()) {
    int cur = 0;
    ZK_HIP(hipGetDevice(&cur));
    devs->push_back(cur);
  }
  return ZK_OK;
}
unsigned devset_turn() { return g_devset_turn.fetch_add(1); }

void host_entry_release_all() {
  bases_cache_release_all();
  stage_pool().release_all([](HostStage& s) {  // (the streams stay: they hold no device memory)
    for (DevBuf* b : {&s.sc[0], &s.sc[1], &s.bases, &s.raw}) b->release();
  });
  DeviceBufPool::pool().release_all([](DeviceBufPool::Buf& b) { b.release(); });
}
}  // namespace zk
