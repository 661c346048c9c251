// The pinned-bases cache of the host-buffer multiexp (bases_cache.hip; SURVEY 8b "Ownership"): the CRS / tau-table is reused across calls
// (`Arc<Vec<G>>` inside groth16::Parameters, groth16/mod.rs:216-238), so the device copy of a base vector the caller has PINNED
// (mi355zk_bases_cache_pin: "this host vector is immutable until I invalidate it" -- the shim holds a clone of the Arc, so the allocation
// can neither be rewritten nor freed and reused) stays on the device, keyed by (host pointer, length, group, layout, device) with a
// fingerprint of sampled records as a safety net; LRU-bounded per device (env MI355ZK_BASES_CACHE_GB, default 64; 0 disables).  Vectors
// that were not pinned are uploaded on every call (env MI355ZK_BASES_CACHE_IMPLICIT=1 restores round 2's behaviour: every vector is
// treated as pinned).  The entries, the pin list and their lock are the unit's own: everything else goes through the functions below.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>
#include <mutex>
#include <vector>

#include "api_internal.hpp"  // RecordLayout

namespace zk {
struct BasesEntry {
  const void* host = nullptr;   // first record of what is cached: the pinned vector itself, or the SLICE of it a multi-GPU cell consumes
  const void* owner = nullptr;  // the pinned vector the records belong to (== host unless a slice): what invalidate / info are asked about
  size_t n = 0;
  int group = 0, dev = 0;
  RecordLayout lay;        // the host records' layout (part of the key: the device copy is always packed)
  uint64_t fp = 0;
  void* d = nullptr;
  size_t bytes = 0;        // of the packed device copy
  uint64_t tick = 0;
  bool ready = false;      // fully uploaded
  std::mutex fill_mu;      // held by the call that uploads it
  // the vector's WINDOW TABLE (table mode, msm_host.hpp), for vectors pinned with mi355zk_bases_cache_pin_tables: built by the first
  // call that finds the entry ready, counted against the cache's capacity, freed with the entry
  bool want_table = false, table_failed = false;
  void* table = nullptr;
  size_t table_bytes = 0;
  size_t table_reserved = 0;  // bytes set aside under the cache's lock while the table is being built (concurrent builds cannot overbook the cache)
  std::mutex table_mu;
};

// the caller's promise of immutability (include/mi355zk.h); lay: the records' layout (part of the pin and of the cache key)
int bases_cache_pin(const void* host, size_t n, int group, bool tables = false, const RecordLayout& lay = RecordLayout());
// The entry of the n records at `host` on device `dev` (locked for filling when *fill == true: the caller uploads and then sets ready) or
// nullptr (cache off / not pinned / no room).  bytes: of the packed device copy; the host records are n * lay.host_stride(group) bytes.
// owner: the vector a multi-GPU cell's slice was cut from (nullptr: the records are the vector itself) -- the owner of an IMPLICITLY
// cached slice, so that mi355zk_bases_cache_invalidate(vector) reaches the slices on every device (a pinned vector's slices
// find their owner in the pin list).
std::shared_ptr<BasesEntry> bases_lookup(const void* host, size_t n, int group, size_t bytes, int dev, bool* fill, const RecordLayout& lay,
                                         const void* owner);
struct FillGuard {  // whatever happens, the entry a call fills is either ready or gone when the call returns
  std::shared_ptr<BasesEntry> e;
  bool fill, ok = false;
  ~FillGuard();
};
// the window table of a ready cache entry whose vector was pinned with tables: built by the first call that asks (the others wait on
// table_mu), inside the cache's capacity (no eviction for it: a table that does not fit is not built and the calls stay plain)
template <int GROUP>
const void* bases_table(const std::shared_ptr<BasesEntry>& e, hipStream_t st);
extern template const void* bases_table<1>(const std::shared_ptr<BasesEntry>&, hipStream_t);
extern template const void* bases_table<2>(const std::shared_ptr<BasesEntry>&, hipStream_t);
// forget the device copies of the base vector at `host` (nullptr: of every vector); entries in use stay until their call ends
void bases_cache_invalidate(const void* host);
int bases_cache_info(const void* host_bases, size_t* device_bytes, size_t* table_bytes);
// the device of the first entry (ready or being filled) that is a copy of the whole vector on one of `devs`, or -1
int bases_cache_device_holding(const void* host, size_t n, int group, const RecordLayout& lay, const std::vector<int>& devs);
void bases_cache_release_all();  // every entry's device memory, in use or not (mi355zk_shutdown)
}  // namespace zk
