// The pinned-bases cache (bases_cache.hpp): the pin list, the entries and their LRU bound per device, the window tables of pinned vectors.
// Host code only -- no kernel is launched from here but through msm_table_build (scalar_mul.hip).
// Locking: g_bc_mu guards the pin list, the entry list and every entry's tick / fingerprint / table accounting; it is never held across a
// fingerprint, an upload or a table build.  An entry's fill_mu is taken UNDER g_bc_mu by the call that creates it and held until its
// upload has ended (FillGuard); a call that finds the entry waits on fill_mu outside g_bc_mu.
#include "bases_cache.hpp"

#include <algorithm>
#include <cstdlib>

namespace zk {
static std::mutex g_bc_mu;
static std::vector<std::shared_ptr<BasesEntry>> g_bc;
static uint64_t g_bc_tick = 0;
// the vectors the caller declared immutable (mi355zk_bases_cache_pin)
struct BasesPin {
  const void* host;
  size_t n;
  int group;
  bool tables;
  RecordLayout lay;
};
static std::vector<BasesPin> g_bc_pins;  // under g_bc_mu

static uint64_t fnv1a(uint64_t h, const uint8_t* p, size_t n) {
  for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 0x100000001b3ull; }
  return h;
}
// first / last 4 KiB and 4096 records spread over the array: cheap (~0.3 MB hashed), and a different CRS at the same address
// is caught; a few records rewritten IN PLACE are not -- which is why caching is OPT-IN: only vectors the caller pinned (declared
// immutable) are served from the device copy, the fingerprint is a second line of defence, not the contract
static uint64_t bases_fingerprint(const uint8_t* p, size_t bytes, size_t rec) {
  uint64_t h = 0xcbf29ce484222325ull;
  const size_t edge = bytes < 4096 ? bytes : 4096;
  h = fnv1a(h, p, edge);
  h = fnv1a(h, p + bytes - edge, edge);
  const size_t nrec = bytes / rec;
  for (size_t k = 1; k <= 4096 && nrec > 0; ++k) h = fnv1a(h, p + (nrec * k / 4097) * rec, rec);
  return h;
}
static size_t bases_cache_cap() {
  static const char* env = std::getenv("MI355ZK_BASES_CACHE_GB");
  const double gb = env ? std::atof(env) : 64.0;
  return gb <= 0 ? 0 : (size_t)(gb * 1073741824.0);
}
static bool bases_cache_implicit() {
  static const char* env = std::getenv("MI355ZK_BASES_CACHE_IMPLICIT");
  return env && env[0] == '1';
}
// the bytes of device `dev` the cache accounts for: copies, tables and the room reserved for tables being built (under g_bc_mu)
static size_t used_on(int dev) {
  size_t used = 0;
  for (auto& x : g_bc)
    if (x->dev == dev) used += x->bytes + x->table_bytes + x->table_reserved;
  return used;
}
// an entry's two device allocations (on the current device: a caller that walks several devices sets the entry's first)
static void free_entry(const BasesEntry& e) {
  (void)hipFree(e.d);
  (void)hipFree(e.table);
}
static bool names(const BasesEntry& e, const void* host) { return host == nullptr || e.host == host || e.owner == host; }  // what invalidate is asked about

int bases_cache_pin(const void* host, size_t n, int group, bool tables, const RecordLayout& lay) {
  if (!host || n == 0 || (group != 1 && group != 2)) return ZK_ERR_BAD_ARGS;
  std::lock_guard<std::mutex> lk(g_bc_mu);
  for (auto& p : g_bc_pins)
    if (p.host == host && p.n == n && p.group == group && p.lay == lay) {
      p.tables = p.tables || tables;
      return ZK_OK;
    }
  g_bc_pins.push_back(BasesPin{host, n, group, tables, lay});
  return ZK_OK;
}

std::shared_ptr<BasesEntry> bases_lookup(const void* host, size_t n, int group, size_t bytes, int dev, bool* fill, const RecordLayout& lay,
                                         const void* owner) {
  *fill = false;
  const size_t cap = bases_cache_cap();
  if (cap == 0 || bytes > cap) return nullptr;
  bool want_table = false;
  if (owner == nullptr) owner = host;
  {
    std::lock_guard<std::mutex> lk(g_bc_mu);
    // pinned: the vector itself, or a record range INSIDE a pinned vector (the single-process multi-GPU mode caches on each device only
    // the slice its cell consumes: SURVEY 8e "the tau-table slice stays resident on its GPU")
    bool pinned = false;
    const size_t rec = lay.host_stride(group);
    for (auto& p : g_bc_pins) {
      if (p.group != group || p.lay != lay) continue;
      const char* lo = (const char*)p.host;
      if ((const char*)host >= lo && (const char*)host + n * rec <= lo + p.n * rec) {
        pinned = true;
        owner = p.host;
        want_table = want_table || (p.tables && p.host == host && p.n == n);   // (tables for whole vectors only: a slice's calls are cells)
      }
    }
    if (!pinned && !bases_cache_implicit()) return nullptr;
  }
  // (the fingerprint is computed OUTSIDE the lock: ~0.3 MB of the caller's memory is read)
  const size_t rec = lay.host_stride(group);  // (strided: whole records are sampled, the flag byte included)
  const uint64_t fp = bases_fingerprint((const uint8_t*)host, n * rec, rec);
  std::shared_ptr<BasesEntry> hit;
  {
    std::lock_guard<std::mutex> lk(g_bc_mu);
    for (auto& e : g_bc)
      if (e->host == host && e->n == n && e->group == group && e->lay == lay && e->dev == dev && e->fp == fp) { hit = e; break; }
    if (hit) { hit->tick = ++g_bc_tick; hit->want_table = hit->want_table || want_table; }
  }
  if (hit) {
    std::lock_guard<std::mutex> wait_fill(hit->fill_mu);  // another thread may still be uploading it
    if (hit->ready) return hit;
    return nullptr;                                       // its upload failed: go uncached
  }
  auto e = std::make_shared<BasesEntry>();
  e->host = host; e->owner = owner; e->n = n; e->group = group; e->lay = lay; e->dev = dev; e->fp = fp; e->bytes = bytes; e->want_table = want_table;
  {
    std::lock_guard<std::mutex> lk(g_bc_mu);
    // the capacity is PER DEVICE (a process may drive several: mi355zk_init with n_devices > 1 keeps a copy of a pinned vector on
    // every device that evaluates cells over it)
    size_t used = used_on(dev);
    while (used + bytes > cap && !g_bc.empty()) {           // evict least recently used entries nobody is filling
      size_t victim = g_bc.size();
      for (size_t i = 0; i < g_bc.size(); ++i)
        if (g_bc[i]->dev == dev && g_bc[i]->ready && g_bc[i].use_count() == 1 && g_bc[i]->table_reserved == 0 &&
            (victim == g_bc.size() || g_bc[i]->tick < g_bc[victim]->tick))
          victim = i;
      if (victim == g_bc.size()) break;
      free_entry(*g_bc[victim]);
      used -= g_bc[victim]->bytes + g_bc[victim]->table_bytes;
      g_bc.erase(g_bc.begin() + (long)victim);
    }
    if (used + bytes > cap) return nullptr;
    if (hipMalloc(&e->d, bytes) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
    e->tick = ++g_bc_tick;
    e->fill_mu.lock();
    g_bc.push_back(e);
  }
  *fill = true;
  return e;
}

static void bases_drop(const std::shared_ptr<BasesEntry>& e) {  // a failed upload
  std::lock_guard<std::mutex> lk(g_bc_mu);
  for (size_t i = 0; i < g_bc.size(); ++i)
    if (g_bc[i] == e) { g_bc.erase(g_bc.begin() + (long)i); break; }
  free_entry(*e);
  e->d = e->table = nullptr;
  e->table_bytes = 0;
}
FillGuard::~FillGuard() {
  if (!fill) return;
  e->ready = ok;
  e->fill_mu.unlock();
  if (!ok) bases_drop(e);
}

void bases_cache_invalidate(const void* host) {
  int cur = 0;
  (void)hipGetDevice(&cur);
  std::lock_guard<std::mutex> lk(g_bc_mu);
  for (size_t i = 0; i < g_bc_pins.size();) {  // the promise of immutability ends here
    if (host == nullptr || g_bc_pins[i].host == host) g_bc_pins.erase(g_bc_pins.begin() + (long)i);
    else ++i;
  }
  for (size_t i = 0; i < g_bc.size();) {
    if (names(*g_bc[i], host) && g_bc[i]->ready && g_bc[i].use_count() == 1) {
      (void)hipSetDevice(g_bc[i]->dev);
      free_entry(*g_bc[i]);
      g_bc.erase(g_bc.begin() + (long)i);
    } else {
      if (names(*g_bc[i], host)) g_bc[i]->fp ^= 0x9e3779b97f4a7c15ull;  // in use: never matched again
      ++i;
    }
  }
  (void)hipSetDevice(cur);
}

int bases_cache_info(const void* host_bases, size_t* device_bytes, size_t* table_bytes) {
  size_t d = 0, t = 0;
  int found = 0;
  {
    std::lock_guard<std::mutex> lk(g_bc_mu);
    for (auto& e : g_bc)
      if ((e->host == host_bases || e->owner == host_bases) && e->ready) { d += e->bytes; t += e->table_bytes; found = 1; }
  }
  if (device_bytes) *device_bytes = d;
  if (table_bytes) *table_bytes = t;
  return found;
}

int bases_cache_device_holding(const void* host, size_t n, int group, const RecordLayout& lay, const std::vector<int>& devs) {
  std::lock_guard<std::mutex> lk(g_bc_mu);
  for (auto& e : g_bc)
    if (e->host == host && e->n == n && e->group == group && e->lay == lay && std::find(devs.begin(), devs.end(), e->dev) != devs.end()) return e->dev;
  return -1;
}

void bases_cache_release_all() {
  std::lock_guard<std::mutex> lk(g_bc_mu);
  for (auto& e : g_bc) { (void)hipSetDevice(e->dev); free_entry(*e); }
  g_bc.clear();
}

template <int GROUP>
const void* bases_table(const std::shared_ptr<BasesEntry>& e, hipStream_t st) {
  if (!e || !e->want_table || !e->ready) return nullptr;
  std::lock_guard<std::mutex> lk(e->table_mu);
  if (e->table) return e->table;
  if (e->table_failed) return nullptr;
  uint32_t c = 0, W = 0;
  msm_table_geometry(e->n, GROUP, &c, &W, nullptr);
  const size_t bytes = (size_t)W * e->bytes;
  if ((uint64_t)W * e->n > 0x7fffffffull) { e->table_failed = true; return nullptr; }
  {
    // reserve the room before the build: the prover's eight threads build the tables of different vectors at the same time.  A
    // cache that is full NOW is not a failure of this vector -- the next call asks again, after evictions may have made room.
    std::lock_guard<std::mutex> g(g_bc_mu);
    if (used_on(e->dev) + bytes > bases_cache_cap()) return nullptr;
    e->table_reserved = bytes;
  }
  void* t = nullptr;
  bool ok = hipMalloc(&t, bytes) == hipSuccess;
  if (!ok) (void)hipGetLastError();
  if (ok && msm_table_build<GROUP>(e->d, e->n, t, bytes, (void*)st) != ZK_OK) { (void)hipFree(t); ok = false; }
  std::lock_guard<std::mutex> g(g_bc_mu);
  e->table_reserved = 0;
  if (!ok) { e->table_failed = true; return nullptr; }  // allocation or build failed: not tried again for this entry
  e->table = t;
  e->table_bytes = bytes;
  return t;
}
template const void* bases_table<1>(const std::shared_ptr<BasesEntry>&, hipStream_t);
template const void* bases_table<2>(const std::shared_ptr<BasesEntry>&, hipStream_t);
}  // namespace zk
