// The state behind host_pools.hpp: the pool of stages, the device set of mi355zk_init, and the release of everything the host-buffer entry
// points keep on the devices.  Host code only.
#include "host_pools.hpp"

#include <atomic>

#include "bases_cache.hpp"

namespace zk {
std::mutex g_stage_mu;
static std::vector<HostStage*> g_stages;  // the pool: as many stages as there have been concurrent host-buffer calls
HostStage* host_stage(int dev) {  // an idle stage of the device, marked busy (nullptr: no streams to be had)
  HostStage* mine = nullptr;
  {
    std::lock_guard<std::mutex> lk(g_stage_mu);
    for (HostStage* s : g_stages)  // the idle stage of this device with the largest staging buffers
      if (!s->busy && s->dev == dev && (mine == nullptr || s->sc[0].bytes + s->sc[1].bytes > mine->sc[0].bytes + mine->sc[1].bytes)) mine = s;
    if (mine) mine->busy = true;
  }
  if (mine == nullptr) {
    mine = new HostStage();
    mine->dev = dev;
    mine->busy = true;
    if (hipStreamCreateWithFlags(&mine->copy, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&mine->compute, hipStreamNonBlocking) != hipSuccess) {
      delete mine;
      return nullptr;
    }
    std::lock_guard<std::mutex> lk(g_stage_mu);
    g_stages.push_back(mine);
  }
  return mine;
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
  std::lock_guard<std::mutex> lk(g_stage_mu);
  for (HostStage* s : g_stages) {
    (void)hipSetDevice(s->dev);
    for (DevBuf* b : {&s->sc[0], &s->sc[1], &s->bases, &s->raw}) b->release();
  }
  std::lock_guard<std::mutex> dl(DeviceBufPool::mu());
  for (DeviceBufPool::Buf* b : DeviceBufPool::all()) {
    (void)hipSetDevice(b->dev);
    b->release();
  }
}
}  // namespace zk
