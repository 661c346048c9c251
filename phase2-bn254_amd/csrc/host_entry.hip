// The multiexp behind the C ABI (include/mi355zk.h): the device-resident call wrapper (msm_dev_entry), the streamed upload of a host-buffer
// multiexp (msm_host_run) and the single-process multi-GPU mode (msm_host_multi).  What they plan -- the Source / QueryDensity arithmetic of
// bellman/src/source.rs, the chunk schedule, the cells and their join -- is host_plan.hpp; the pinned-bases cache is bases_cache.hpp, stages
// and the device set host_pools.hpp; the other host-buffer entry points are host_ops.hip; the extern "C" wrappers stay in api.hip.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <condition_variable>
#include <cstdio>
#include <cstring>
#include <memory>
#include <mutex>
#include <thread>
#include <type_traits>
#include <vector>

#include "../../include/mi355zk.h"
#include "curveu.hpp"
#include "api_internal.hpp"
#include "bases_cache.hpp"
#include "host_plan.hpp"
#include "host_pools.hpp"

namespace zk {
thread_local long long t_last_err_index = -1;

template <int GROUP>
int msm_dev_entry(const void* d_bases, size_t n_bases, size_t base_offset, const void* d_scalars, size_t n_scalars,
                  const uint32_t* density, size_t density_bits, void* stream, uint64_t* out_xyz, uint32_t wgroups, uint32_t wgroup,
                  uint32_t flags, MsmChunks* chunks, bool table) {
  // table: d_bases is the window table msm_table_build made of a vector of n_bases points (table mode, msm_host.hpp)
  // chunks != nullptr: the exponents are handed over chunk by chunk while the call runs (msm_host_entry); d_scalars is unused
  t_last_err_index = -1;
  if (!out_xyz || (n_scalars && !d_scalars && !chunks) || (n_bases && !d_bases)) return ZK_ERR_BAD_ARGS;
  if (n_bases >= (1ull << 31) || n_scalars >= (1ull << 31)) return ZK_ERR_BAD_ARGS;
  hipStream_t st = (hipStream_t)stream;
  const DensityPlan P = plan_density(n_bases, base_offset, n_scalars, density, density_bits);
  const uint64_t n = P.live();
  int rc = ZK_OK;
  uint32_t* d_density = nullptr;
  uint32_t* d_prefix = nullptr;
  DeviceBufPool::Lease density_lease;
  if (density != nullptr && n > 0) {
    // the device copy of the map (words + prefix popcounts), leased on the caller's stream for the duration of the call (a buffer per
    // host thread would outlive short-lived caller threads)
    int dev = 0;
    ZK_HIP(hipGetDevice(&dev));
    size_t words = (n + 31) / 32;
    rc = density_lease.acquire(dev, words * 8, st);
    if (rc) return rc;
    d_density = (uint32_t*)density_lease.p();
    d_prefix = d_density + words;
    ZK_HIP(hipMemcpyAsync(d_density, density, words * 4, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_prefix, P.prefix.data(), words * 4, hipMemcpyHostToDevice, st));
  }
  long long err_index = -1;
  const bool mont = (flags & MI355ZK_MSM_SCALARS_MONTGOMERY) != 0;
  if (chunks && (chunks->n_chunks == 0 || chunks->cuts[chunks->n_chunks] != n)) return ZK_ERR_BAD_ARGS;
  uint32_t tc = 0, tW = 0;
  if (table) msm_table_geometry(n_bases, GROUP, &tc, &tW, nullptr);
  const uint64_t tstride = table ? (uint64_t)n_bases : 0;
  if (table && n_bases == 0 && n > 0) return ZK_ERR_BAD_ARGS;
  if (GROUP == 1) rc = msm_g1_device(d_bases, n_bases, base_offset, d_scalars, n, d_density, d_prefix, st, out_xyz, &err_index, wgroups, wgroup, mont, chunks, tstride, tc);
  else rc = msm_g2_device(d_bases, n_bases, base_offset, d_scalars, n, d_density, d_prefix, st, out_xyz, &err_index, wgroups, wgroup, mont, chunks, tstride, tc);
  if (rc == ZK_ERR_UNEXPECTED_IDENTITY) {
    // the kernels report the lowest BASE index that was the identity under a non-zero exponent; the exponent that owns it
    // is the (index - base_offset)-th selected one (source.rs:101-118): itself under FullDensity
    t_last_err_index = (long long)P.select((uint64_t)(err_index - (long long)base_offset));
    return rc;
  }
  if (rc == ZK_ERR_BAD_ARGS) t_last_err_index = err_index;  // a non-canonical exponent (>= 2^254): its index
  if (rc != ZK_OK) return rc;
  if (P.eof_index >= 0) { t_last_err_index = P.eof_index; return ZK_ERR_UNEXPECTED_EOF; }
  return ZK_OK;
}

// A batch of exponent vectors over one base vector (msm_host.hpp: msm_device_batch).  The Source / density arithmetic belongs to the base vector
// and the map, so it is done once; a vector's Source error is translated as msm_dev_entry translates it.  Exponents beyond the bases
// (UnexpectedEof) are every vector's error unless the vector has an earlier one: the single call decides, vector by vector.
template <int GROUP>
int msm_batch_dev_entry(const void* d_bases, size_t n_bases, size_t base_offset, const void* d_scalars, size_t n_scalars, size_t scalar_stride,
                        size_t n_vectors, const uint32_t* density, size_t density_bits, uint32_t flags, void* stream, uint64_t* out_xyz, int* rcs,
                        long long* err_indices) {
  t_last_err_index = -1;
  constexpr size_t words = GROUP == 1 ? 12 : 24;
  if (!out_xyz || !rcs || !err_indices || n_vectors == 0 || scalar_stride < n_scalars || (n_scalars && !d_scalars) || (n_bases && !d_bases)) return ZK_ERR_BAD_ARGS;
  if (n_bases >= (1ull << 31) || n_scalars >= (1ull << 31) || scalar_stride >= (1ull << 31) || n_vectors >= (1ull << 31)) return ZK_ERR_BAD_ARGS;
  if (flags & ~MI355ZK_MSM_SCALARS_MONTGOMERY) return ZK_ERR_BAD_ARGS;
  const DensityPlan P = plan_density(n_bases, base_offset, n_scalars, density, density_bits);
  if (P.eof_index >= 0 || n_vectors == 1) {
    for (size_t v = 0; v < n_vectors; ++v) {
      rcs[v] = msm_dev_entry<GROUP>(d_bases, n_bases, base_offset, (const char*)d_scalars + v * scalar_stride * 32, n_scalars, density, density_bits, stream,
                                    out_xyz + v * words, 1, 0, flags);
      err_indices[v] = t_last_err_index;
    }
    return ZK_OK;
  }
  hipStream_t st = (hipStream_t)stream;
  const uint64_t n = P.live();
  uint32_t* d_density = nullptr;
  uint32_t* d_prefix = nullptr;
  DeviceBufPool::Lease density_lease;
  if (density != nullptr && n > 0) {
    int dev = 0;
    ZK_HIP(hipGetDevice(&dev));
    const size_t dwords = (n + 31) / 32;
    if (int rc = density_lease.acquire(dev, dwords * 8, st)) return rc;
    d_density = (uint32_t*)density_lease.p();
    d_prefix = d_density + dwords;
    ZK_HIP(hipMemcpyAsync(d_density, density, dwords * 4, hipMemcpyHostToDevice, st));
    ZK_HIP(hipMemcpyAsync(d_prefix, P.prefix.data(), dwords * 4, hipMemcpyHostToDevice, st));
  }
  const bool mont = (flags & MI355ZK_MSM_SCALARS_MONTGOMERY) != 0;
  int rc;
  if (GROUP == 1) rc = msm_g1_batch_device(d_bases, n_bases, base_offset, d_scalars, n, scalar_stride, (uint32_t)n_vectors, d_density, d_prefix, st, out_xyz, rcs, err_indices, mont);
  else rc = msm_g2_batch_device(d_bases, n_bases, base_offset, d_scalars, n, scalar_stride, (uint32_t)n_vectors, d_density, d_prefix, st, out_xyz, rcs, err_indices, mont);
  if (rc != ZK_OK) return rc;
  for (size_t v = n_vectors; v-- > 0;) {
    if (rcs[v] == ZK_ERR_UNEXPECTED_IDENTITY) err_indices[v] = (long long)P.select((uint64_t)(err_indices[v] - (long long)base_offset));   // (msm_dev_entry)
    else if (rcs[v] != ZK_ERR_BAD_ARGS) err_indices[v] = -1;
    if (rcs[v] != ZK_OK) t_last_err_index = err_indices[v];   // (the thread's last-error index: the first failing vector's)
  }
  return ZK_OK;
}

// ------------------------------------------------------------------------------------------------
// Host-buffer entry points (SURVEY 8b "Ownership"): the caller's bases and scalars live in (pageable) host memory.
//   * BASES CACHE (bases_cache.hpp): the device copy of a base vector the caller has PINNED stays on the device; vectors that were not
//     pinned are uploaded on every call.
//   * STREAMED UPLOAD: a large call is cut into chunks of ~2^24 exponents (host_plan.hpp: host_chunk_cuts); a copy thread uploads chunk
//     i + 1 (its scalars into one of two staging buffers, its bases -- when they are not cached yet -- straight into the cache entry) on a
//     copy stream while the calling thread runs the multiexp of chunk i on a compute stream; the Jacobian partials are added on the host.
//     PCIe and the kernels overlap; the first call is bound by the link (96 B per exponent), later calls by the kernels.

// Host records [lo, hi) of a base vector -> the packed device copy, enqueued on the stage's copy stream.  Packed records go straight over the
// link.  Strided records go raw, in pieces of at most RAW_PIECE records, into the stage's raw buffer, and records_pack repacks each piece into
// the copy behind its upload; the copy stream's order keeps a piece from overwriting the raw buffer before the previous piece's repack has
// read it.  The device memory on top of the packed copy is one piece, not the vector.
constexpr uint64_t RAW_PIECE = 1ull << 19;
struct BaseUpload {
  const uint8_t* host;
  void* dev;
  int group;
  const RecordLayout& L;
  HostStage* S;
  hipError_t put(uint64_t lo, uint64_t hi) const {
    if (hi <= lo) return hipSuccess;
    const size_t bsz = group == 1 ? 64 : 128, hs = L.host_stride(group);
    if (L.packed()) return hipMemcpyAsync((char*)dev + lo * bsz, host + lo * bsz, (hi - lo) * bsz, hipMemcpyHostToDevice, S->copy);
    for (uint64_t p = lo; p < hi; p += RAW_PIECE) {
      const uint64_t m = std::min<uint64_t>(RAW_PIECE, hi - p);
      hipError_t e = hipMemcpyAsync(S->raw.p, host + p * hs, m * hs, hipMemcpyHostToDevice, S->copy);
      if (e != hipSuccess) return e;
      if (records_pack_run(group, S->raw.p, m, L, (char*)dev + p * bsz, S->copy) != ZK_OK) return hipErrorLaunchFailure;
    }
    return hipSuccess;
  }
};

// What the compute side (msm_device through MsmChunks) and the copy thread of a streamed call share.  staging[c & 1] is free again once the
// DIGIT kernel of chunk c - 2 -- the only reader of a chunk's exponents -- has run: the compute side records an event behind it.
struct Feed : MsmChunks {
  std::mutex mu;
  std::condition_variable cv;
  uint64_t copied = 0, digits = 0;          // chunks uploaded / chunks whose digit kernel has been enqueued
  bool copy_failed = false, abort_copy = false;
  void* sc[2];
  Events ev;                                // ev[c]: recorded behind chunk c's digit kernel
  Feed(const std::vector<uint64_t>& chunk_cuts, const HostStage* S) : sc{S->sc[0].p, S->sc[1].p}, ev(chunk_cuts.size() - 1) {
    n_chunks = (uint32_t)(chunk_cuts.size() - 1);
    cuts = chunk_cuts.data();
  }
  int acquire(uint32_t c, hipStream_t, const void** d) override {
    std::unique_lock<std::mutex> lk(mu);
    cv.wait(lk, [&] { return copy_failed || copied > c; });  // (a host-side wait: the earlier chunks' kernels are already queued)
    if (copy_failed) return ZK_ERR_DEVICE;
    *d = sc[c & 1];
    return ZK_OK;
  }
  int digits_enqueued(uint32_t c, hipStream_t st) override {
    ZK_HIP(hipEventRecord(ev[c], st));
    std::lock_guard<std::mutex> lk(mu);
    digits = c + 1;
    cv.notify_all();
    return ZK_OK;
  }
};

// The copy thread: for chunk c, scalars -> staging[c & 1] and (when uploading) the bases the chunk consumes; afterwards (complete_entry) the
// bases outside the consumed range, so that a cache entry is complete.
struct CopyJob {
  int dev;
  const uint64_t* scalars;
  const DensityPlan& P;
  uint64_t n_bases, base_offset;
  bool upload_bases, complete_entry;
  const BaseUpload& up;
  std::chrono::steady_clock::time_point t0;
};
void copy_chunks(Feed& feed, const CopyJob& J) {
  auto fail = [&] { std::lock_guard<std::mutex> lk(feed.mu); feed.copy_failed = true; feed.cv.notify_all(); };
  if (hipSetDevice(J.dev) != hipSuccess) { fail(); return; }
  hipStream_t copy = J.up.S->copy;
  const uint64_t b_lo = J.base_offset < J.n_bases ? J.base_offset : J.n_bases;
  uint64_t b_done = b_lo;  // bases [b_lo, b_done) are on the device
  for (uint64_t c = 0; c < feed.n_chunks; ++c) {
    if (c >= 2) {
      {
        std::unique_lock<std::mutex> lk(feed.mu);
        feed.cv.wait(lk, [&] { return feed.abort_copy || feed.digits >= c - 1; });
        if (feed.abort_copy) return;
      }
      if (hipEventSynchronize(feed.ev[c - 2]) != hipSuccess) { fail(); return; }
    } else {
      std::lock_guard<std::mutex> lk(feed.mu);
      if (feed.abort_copy) return;
    }
    const uint64_t lo = feed.cuts[c], hi = feed.cuts[c + 1];
    hipError_t e = hipMemcpyAsync(feed.sc[c & 1], J.scalars + lo * 4, (hi - lo) * 32, hipMemcpyHostToDevice, copy);
    if (e == hipSuccess && J.upload_bases) {
      uint64_t b_hi = J.base_offset + J.P.rank(hi);
      if (b_hi > J.n_bases) b_hi = J.n_bases;
      if (b_hi > b_done) {
        e = J.up.put(b_done, b_hi);
        b_done = b_hi;
      }
    }
    if (e == hipSuccess) e = hipStreamSynchronize(copy);
    if (e != hipSuccess) { fail(); return; }
    if (trace_host()) std::fprintf(stderr, "[mi355zk] host entry: chunk %llu (%llu exponents) uploaded at %.2f ms\n", (unsigned long long)c, (unsigned long long)(hi - lo), ms_since(J.t0));
    std::lock_guard<std::mutex> lk(feed.mu);
    feed.copied = c + 1;
    feed.cv.notify_all();
  }
  if (J.complete_entry) {  // the rest of the vector (not needed by this call) completes the cache entry
    hipError_t e = hipSuccess;
    if (b_lo > 0) e = J.up.put(0, b_lo);
    if (e == hipSuccess && b_done < J.n_bases) e = J.up.put(b_done, J.n_bases);
    if (e == hipSuccess) e = hipStreamSynchronize(copy);
    if (e != hipSuccess) fail();
  }
}

// One host-buffer multiexp on the calling thread's CURRENT device.  (wgroups, wgroup): only that group of scalar windows (a cell of
// the single-process multi-GPU mode below; (1, 0) is the whole multiexp).
// L: the layout of the host records (strided records are repacked on the device as they arrive).  K: the call's knobs (msm_host_entry reads
// them).  owner: the vector `bases` is a slice of (a cell's call; nullptr: the vector itself) -- what the cache files the slice under.
template <int GROUP>
int msm_host_run(const uint8_t* bases, size_t n_bases, size_t base_offset, const uint64_t* scalars, size_t n_scalars,
                 const uint32_t* density, size_t density_bits, uint64_t* out_xyz, const HostKnobs& K, const RecordLayout& L,
                 const void* owner = nullptr, uint32_t wgroups = 1, uint32_t wgroup = 0) {
  t_last_err_index = -1;
  if (!msm_host_args_ok(bases, n_bases, scalars, n_scalars, out_xyz)) return ZK_ERR_BAD_ARGS;
  constexpr size_t bsz = GROUP == 1 ? 64 : 128;
  constexpr size_t jac_words = GROUP == 1 ? 12 : 24;
  int dev = 0;
  ZK_HIP(hipGetDevice(&dev));
  CallLease lease;
  int rc = lease.open(dev);
  if (rc) return rc;
  HostStage* S = lease.S;

  // ---- plan: the exponents this call evaluates and the bases they consume (source.rs:36-118)
  const DensityPlan P = plan_density(n_bases, base_offset, n_scalars, density, density_bits);
  const uint64_t n = P.live();

  // ---- bases: cached, being cached by this call, or (not pinned / cache off / full) the leased stage's buffer
  bool fill = false;
  std::shared_ptr<BasesEntry> entry = n_bases ? bases_lookup(bases, n_bases, GROUP, n_bases * bsz, dev, &fill, L, owner) : nullptr;
  void* d_bases = entry ? entry->d : nullptr;
  bool upload_bases = fill;
  if (!entry && n_bases) {
    rc = S->bases.reserve(n_bases * bsz);
    if (rc) return rc;
    d_bases = S->bases.p;
    upload_bases = true;
  }
  FillGuard guard{entry, fill};
  if (!L.packed() && n_bases && upload_bases) {
    rc = S->raw.reserve((size_t)std::min<uint64_t>(n_bases, RAW_PIECE) * L.host_stride(GROUP));
    if (rc) return rc;
  }
  const BaseUpload up{bases, d_bases, GROUP, L, S};

  // ---- cuts, and the two staging buffers of the largest chunk
  const std::vector<uint64_t> cuts = host_chunk_cuts(n, upload_bases, K);
  const uint64_t n_chunks = cuts.size() - 1;
  uint64_t max_chunk = 0;
  for (uint64_t c = 0; c < n_chunks; ++c) max_chunk = std::max(max_chunk, cuts[c + 1] - cuts[c]);
  for (int k = 0; k < 2 && n; ++k) {
    rc = S->sc[k].reserve((size_t)max_chunk * 32);
    if (rc) return rc;
  }

  // ---- feed
  Feed feed(cuts, S);
  ZK_HIP(feed.ev.create());
  const CopyJob job{dev, scalars, P, n_bases, base_offset, upload_bases, upload_bases && entry, up, std::chrono::steady_clock::now()};

  // ---- run
  uint64_t result_xyz[jac_words];
  {
    // a call that evaluates no exponent returns the reference's Projective::zero() = (0, 1, 0) (ec.rs:229-235), as msm_device does
    using J = typename std::conditional<GROUP == 1, G1Jacobian, G2Jacobian>::type;
    static_assert(sizeof(J) == sizeof result_xyz, "Jacobian layout");
    const J zero = J::zero();
    std::memcpy(result_xyz, &zero, sizeof result_xyz);
  }
  int result = ZK_OK;
  long long err_idx = -1;
  bool aborted = false;
  if (n_chunks > 0) {
    std::thread copier([&] { copy_chunks(feed, job); });
    // a vector pinned WITH TABLES, already on the device, in a call that is not cut: table mode
    // (not for a handful of exponents over a long vector -- the prover's input multiexps over its 2^20-point a / b queries: the
    // table's window width comes from the VECTOR's length, and zeroing + reducing 2^19 buckets for a few points costs more than the
    // plain call, which picks its window from n)
    const bool table_pays = n * 8 >= n_bases;
    const void* d_table = (n_chunks == 1 && entry && !fill && wgroups == 1 && table_pays) ? bases_table<GROUP>(entry, S->compute) : nullptr;
    result = msm_dev_entry<GROUP>(d_table ? d_table : d_bases, n_bases, base_offset, nullptr, n_scalars, density, density_bits, (void*)S->compute, result_xyz,
                                  wgroups, wgroup, 0, &feed, d_table != nullptr);
    err_idx = t_last_err_index;
    if (trace_host()) std::fprintf(stderr, "[mi355zk] host entry: result at %.2f ms (%llu chunks)\n", ms_since(job.t0), (unsigned long long)n_chunks);
    {
      std::lock_guard<std::mutex> lk(feed.mu);
      // a call that failed before it had taken every chunk leaves the copy thread waiting: release it
      aborted = result != ZK_OK && result != ZK_ERR_UNEXPECTED_EOF && feed.digits < n_chunks;
      feed.abort_copy = aborted;
      feed.cv.notify_all();
    }
    copier.join();
    if (feed.copy_failed) result = ZK_ERR_DEVICE;
  } else if (job.complete_entry && n_bases) {
    // nothing to evaluate, but the entry was created: fill it
    hipError_t e = up.put(0, n_bases);
    if (e == hipSuccess) e = hipStreamSynchronize(S->copy);
    if (e != hipSuccess) result = ZK_ERR_DEVICE;
    if (result == ZK_OK && P.eof_index >= 0) { result = ZK_ERR_UNEXPECTED_EOF; err_idx = P.eof_index; }
  } else if (P.eof_index >= 0) {
    result = ZK_ERR_UNEXPECTED_EOF;
    err_idx = P.eof_index;
  }

  // ---- join
  guard.ok = result != ZK_ERR_DEVICE && !feed.copy_failed && !(fill && aborted);  // an aborted streamed upload is incomplete
  t_last_err_index = err_idx;
  if (result != ZK_OK && result != ZK_ERR_UNEXPECTED_EOF) return result;
  std::memcpy(out_xyz, result_xyz, sizeof result_xyz);
  return result;
}

// ------------------------------------------------------------------------------------------------
// SINGLE-PROCESS MULTI-GPU MODE.  The consumer this library is a drop-in for is ONE Rust process (phase2/src/bin/prove.rs ->
// bellman/src/groth16/prover.rs:250-298 -> multiexp.rs:330-355), so the 8 GPUs of a node must be reachable through the C ABI, not
// only through one rank per GPU (shard.py).  mi355zk_init(ids, n > 1) records a DEVICE SET; a host-buffer multiexp of at least
// 2^MI355ZK_MULTI_MIN_LOG exponents (default 20) is then cut into cells -- contiguous POINT RANGES (cut at multiples of 32
// exponents so that density words are not shared), optionally x groups of scalar windows -- and every cell is one msm_host_run on
// its own device from its own host thread: its exponents cross ITS PCIe link while its kernels run (the streamed upload above), its
// base vector is cached on that device when the caller pinned it.  The N Jacobian partials (96 / 192 B) come back to the host --
// SURVEY 8e's "or D2H of 8 records": inside one process there is nothing for RCCL to do -- and are joined there with the rule
// shard.exchange defines: a failing cell's error carries its GLOBAL exponent index, the lowest index wins, Eof (planned for the whole
// call) before identity at one index.  Smaller calls run whole, on the devices of the set in turn (the prover's eight concurrent
// multiexps spread over the node).
// Why point ranges and not shard.py's window groups: a rank of shard.py holds its exponents in HBM; here every cell uploads its own,
// and a window-group cell would upload ALL exponents of its range over its link (2^26 on 8 devices: 1 GiB per device against 256 MiB).
// MI355ZK_MULTI_PLAN="PxW" forces P point ranges x W window groups (P * W <= devices) for experiments and for the tests.
template <int GROUP>
int msm_host_multi(const std::vector<int>& devs, const uint8_t* bases, size_t n_bases, size_t base_offset, const uint64_t* scalars,
                   size_t n_scalars, const uint32_t* density, size_t density_bits, uint64_t* out_xyz, const HostKnobs& K, const RecordLayout& L) {
  using J = typename std::conditional<GROUP == 1, G1Jacobian, G2Jacobian>::type;
  t_last_err_index = -1;
  const DensityPlan P = plan_density(n_bases, base_offset, n_scalars, density, density_bits);
  // ---- the plan: point ranges x window groups
  const CellPlan C = plan_cells(P, base_offset, devs.size(), K, msm_knobs());
  const size_t n_cells = C.cells.size();
  std::vector<J> part(n_cells, J::zero());
  std::vector<long long> err(n_cells, -1);
  const auto t0 = std::chrono::steady_clock::now();
  auto run_cell = [&](size_t i) {
    const HostCell& c = C.cells[i];
    const int dev = devs[c.slot];
    if (hipSetDevice(dev) != hipSuccess) return ZK_ERR_DEVICE;
    // The cell sees only the SLICE of the base vector its exponents consume -- [boff, boff + used) -- as a vector of its own: that is what
    // its device allocates, uploads and (inside a pinned vector) keeps: 2^26 G1 points on 8 devices are 512 MiB per device, not 4 GiB
    // (SURVEY 8e).  The slice is filed under the vector it was cut from, so that an invalidate of the vector reaches it.
    const size_t hs = L.host_stride(GROUP);  // bytes per host record
    const int rc = msm_host_run<GROUP>(bases + c.boff * hs, c.used, 0, scalars + c.lo * 4, c.hi - c.lo, density ? density + (c.lo >> 5) : nullptr,
                                       density ? c.hi - c.lo : 0, reinterpret_cast<uint64_t*>(&part[i]), K, L, bases, C.wg, c.wgi);
    err[i] = t_last_err_index;
    if (trace_host())
      std::fprintf(stderr, "[mi355zk] multi: cell [%llu, %llu) window group %u/%u on device %d: rc %d at %.2f ms\n", (unsigned long long)c.lo,
                   (unsigned long long)c.hi, c.wgi, C.wg, dev, rc, ms_since(t0));
    return rc;
  };
  const std::vector<int> rcs = fan_out(n_cells, run_cell);
  // ---- the join (host_plan.hpp: join_cells); the Jacobian partials of a call that evaluated its exponents are added here
  std::vector<uint64_t> lo(n_cells);
  for (size_t i = 0; i < n_cells; ++i) lo[i] = C.cells[i].lo;
  const CellJoin j = join_cells(rcs.data(), err.data(), lo.data(), n_cells, P.eof_index);
  if (j.rc < 0) return j.rc;   // (a device failure names no exponent)
  t_last_err_index = j.index;
  if (j.rc != ZK_OK && j.rc != ZK_ERR_UNEXPECTED_EOF) return j.rc;
  J total = J::zero();
  for (const J& p : part) jac_add(total, p);
  std::memcpy(out_xyz, &total, sizeof total);
  return j.rc;
}

// the host-buffer entry points: whole on one device, or cut into cells over the device set
template <int GROUP>
int msm_host_entry(const uint8_t* bases, size_t n_bases, size_t base_offset, const uint64_t* scalars, size_t n_scalars,
                   const uint32_t* density, size_t density_bits, uint64_t* out_xyz, const RecordLayout& L) {
  const HostKnobs K = host_knobs();  // (read per call: the tests and the chunk experiments change them inside one process)
  // (the raw set, not devset_or_current: none or one device means "whole, on the CALLER's current device", which need not be the set's)
  const std::vector<int> devs = devset_snapshot();
  if (devs.size() <= 1) return msm_host_run<GROUP>(bases, n_bases, base_offset, scalars, n_scalars, density, density_bits, out_xyz, K, L);
  if (!msm_host_args_ok(bases, n_bases, scalars, n_scalars, out_xyz)) {
    t_last_err_index = -1;
    return ZK_ERR_BAD_ARGS;
  }
  if (n_scalars >= (1ull << K.multi_min_log) && n_scalars >= 64)
    return msm_host_multi<GROUP>(devs, bases, n_bases, base_offset, scalars, n_scalars, density, density_bits, out_xyz, K, L);
  // A short call runs whole on ONE device: the one that already holds the (pinned) vector if there is one -- the device copy of a
  // parameter vector is then made once per process, not once per device of the set (8 x 4 GiB for a 2^26-point CRS) -- else the next in
  // turn, so that the prover's concurrent multiexps over its different vectors spread over the node on first touch.
  int pick = bases_cache_device_holding(bases, n_bases, GROUP, L, devs);
  if (pick < 0) pick = devs[devset_turn() % devs.size()];
  DeviceGuard guard;
  ZK_HIP(hipSetDevice(pick));
  return msm_host_run<GROUP>(bases, n_bases, base_offset, scalars, n_scalars, density, density_bits, out_xyz, K, L);
}

template int msm_batch_dev_entry<1>(const void*, size_t, size_t, const void*, size_t, size_t, size_t, const uint32_t*, size_t, uint32_t, void*, uint64_t*, int*, long long*);
template int msm_batch_dev_entry<2>(const void*, size_t, size_t, const void*, size_t, size_t, size_t, const uint32_t*, size_t, uint32_t, void*, uint64_t*, int*, long long*);
template int msm_dev_entry<1>(const void*, size_t, size_t, const void*, size_t, const uint32_t*, size_t, void*, uint64_t*, uint32_t, uint32_t, uint32_t, MsmChunks*, bool);
template int msm_dev_entry<2>(const void*, size_t, size_t, const void*, size_t, const uint32_t*, size_t, void*, uint64_t*, uint32_t, uint32_t, uint32_t, MsmChunks*, bool);
template int msm_host_entry<1>(const uint8_t*, size_t, size_t, const uint64_t*, size_t, const uint32_t*, size_t, uint64_t*, const RecordLayout&);
template int msm_host_entry<2>(const uint8_t*, size_t, size_t, const uint64_t*, size_t, const uint32_t*, size_t, uint64_t*, const RecordLayout&);
}  // namespace zk
