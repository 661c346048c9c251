#pragma once
// The host-side PLANS of the host-buffer entry points (host_entry.hip, host_ops.hip): the Source / QueryDensity arithmetic of
// bellman/src/source.rs, the chunk schedule of a streamed multiexp, the cells of the single-process multi-GPU mode and the rule that joins
// their outcomes, the row cuts of the QAP matvec and the shared-upload test of merge_pairs -- pure arithmetic on the call's sizes and the
// knobs.  No HIP call and no getenv below host_knobs(): the planners run, and are tested, without a device (tests/test_host_plan_host.py).
#include <stdint.h>

#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_util.hpp"
#include "msm_plan.hpp"

namespace zk {

// Source / QueryDensity contract (source.rs:36-118, multiexp.rs:92): the number of exponents to process, the exponent index of the
// first UnexpectedEof (or -1) and, for a density map, the per-word exclusive prefix popcounts (one entry past the last word: the total).
struct DensityPlan {
  uint64_t n = 0;
  long long eof_index = -1;
  const uint32_t* density = nullptr;  // the caller's map (nullptr: FullDensity)
  std::vector<uint32_t> prefix;
  uint64_t live() const { return eof_index >= 0 ? (uint64_t)eof_index : n; }  // exponents before the first Eof
  // word w of the map without the bits of exponents >= n (the last word of an n that is no multiple of 32)
  uint32_t word(uint64_t w) const { return (w + 1) * 32 > n ? density[w] & ((1u << (n & 31)) - 1u) : density[w]; }
  // bases consumed by exponents [0, i), i <= n (i itself under FullDensity)
  uint64_t rank(uint64_t i) const {
    if (density == nullptr) return i;
    const uint64_t r = prefix[i >> 5];
    return (i & 31) ? r + (uint32_t)__builtin_popcount(word(i >> 5) & ((1u << (i & 31)) - 1u)) : r;
  }
  // the exponent that owns the r-th selected base (r itself under FullDensity); n when fewer than r + 1 bases are selected
  uint64_t select(uint64_t r) const {
    if (density == nullptr) return r;
    if (r >= prefix.back()) return n;
    uint64_t w = 0;
    while (w + 2 < prefix.size() && prefix[w + 1] <= r) ++w;
    uint32_t v = word(w);
    for (uint64_t k = r - prefix[w]; k && v; --k) v &= v - 1;  // drop the set bits below the (r - prefix[w])-th
    return w * 32 + (v ? (uint32_t)__builtin_ctz(v) : 32);
  }
};

inline DensityPlan plan_density(size_t n_bases, size_t base_offset, size_t n_scalars, const uint32_t* density, size_t density_bits) {
  DensityPlan P;
  P.density = density;
  P.n = n_scalars;
  if (density != nullptr && density_bits < P.n) P.n = density_bits;  // zip() stops at the shorter (multiexp.rs:92)
  const uint64_t avail = base_offset < n_bases ? n_bases - base_offset : 0;
  if (density == nullptr) {
    if (P.n > avail) P.eof_index = (long long)avail;
    return P;
  }
  const uint64_t words = (P.n + 31) / 32;
  P.prefix.resize(words + 1);
  uint64_t used = 0;
  for (uint64_t w = 0; w < words; ++w) {
    P.prefix[w] = (uint32_t)used;
    used += (uint32_t)__builtin_popcount(P.word(w));
  }
  P.prefix[words] = (uint32_t)used;
  if (used > avail) P.eof_index = (long long)P.select(avail);  // the (avail + 1)-th selected exponent is the first without a base
  return P;
}

// the argument rules of the host-buffer multiexp (include/mi355zk.h: rc 3)
inline bool msm_host_args_ok(const void* bases, size_t n_bases, const void* scalars, size_t n_scalars, const void* out_xyz) {
  return out_xyz && (!n_scalars || scalars) && (!n_bases || bases) && n_bases < (1ull << 31) && n_scalars < (1ull << 31);
}

// The environment knobs of the host-buffer entry points' plans, read in ONE place (host_knobs) on EVERY call: the tests and
// tools/exp_host_chunks.py change them inside one process.  The planners below take them as an argument.  The defaults are what an empty
// environment gives.  (MI355ZK_BASES_CACHE_GB / _IMPLICIT: bases_cache.hip, MI355ZK_TRACE_HOST: host_pools.hpp -- once per process.)
struct HostKnobs {
  double chunk_growth = 1.8;      // MI355ZK_HOST_CHUNK_GROWTH: percent (>= 100) a chunk may grow over its predecessor (bases on the device)
  int chunk_first_log = 0;        // MI355ZK_HOST_CHUNK_FIRST: log2 (16 .. 30) of the first chunk (bases on the device); 0: by size
  // test hook: MI355ZK_HOST_CHUNK_TEST = exponents per chunk, a multiple of 32 -- cuts calls of ANY size, so that the chunked path can be
  // held against the CPU oracle at sizes the oracle finishes in seconds (0: off)
  uint64_t chunk_test = 0;
  uint32_t plan_p = 0, plan_w = 0;  // MI355ZK_MULTI_PLAN = "PxW": P point ranges x W window groups (0, 0: none asked for)
  int multi_min_log = 20;         // MI355ZK_MULTI_MIN_LOG (0 .. 30): calls of at least 2^this exponents are cut into cells (the tests lower it)
  size_t dense_piece = (size_t)1 << 22;  // MI355ZK_DENSE_PIECE_TEST (>= 16; test hook): points per piece of dense_host, so that the cut can be held against the oracle
};

inline HostKnobs host_knobs() {
  HostKnobs K;
  if (const char* s = std::getenv("MI355ZK_HOST_CHUNK_GROWTH"))
    if (std::atoi(s) >= 100) K.chunk_growth = std::atoi(s) / 100.0;
  if (const char* s = std::getenv("MI355ZK_HOST_CHUNK_FIRST"))
    if (std::atoi(s) >= 16 && std::atoi(s) <= 30) K.chunk_first_log = std::atoi(s);
  if (const char* s = std::getenv("MI355ZK_HOST_CHUNK_TEST")) {
    const uint64_t v = (uint64_t)std::strtoull(s, nullptr, 10) & ~31ull;
    if (v >= 32) K.chunk_test = v;
  }
  if (const char* s = std::getenv("MI355ZK_MULTI_PLAN")) {
    unsigned a = 0, b = 0;
    if (std::sscanf(s, "%ux%u", &a, &b) == 2 && a >= 1 && b >= 1) { K.plan_p = a; K.plan_w = b; }
  }
  if (const char* s = std::getenv("MI355ZK_MULTI_MIN_LOG")) {
    const int v = std::atoi(s);
    K.multi_min_log = v < 0 ? 0 : v > 30 ? 30 : v;
  }
  if (const char* s = std::getenv("MI355ZK_DENSE_PIECE_TEST")) {
    const size_t v = (size_t)std::strtoull(s, nullptr, 10);
    if (v >= 16) K.dense_piece = v;
  }
  return K;
}

constexpr uint64_t HOST_CHUNK_UPLOAD = 1ull << 23;  // exponents per chunk of a streamed call whose bases travel too (link-bound)
constexpr uint64_t HOST_CHUNK_MIN = 1ull << 21;     // smallest first chunk of a call whose bases are on the device; below 4 of these the call is not cut

// The chunk schedule of a streamed call of n exponents: cuts[c] .. cuts[c + 1] is chunk c (cut at multiples of 32 exponents, so that density
// words are not shared between chunks; n == 0: no chunk).  Every chunk runs digits -> partition -> accumulate into the ONE bucket array of
// the call (msm_device, MsmChunks); what a chunk costs on top of its share of the work is the re-partition of the bucket bounds and one
// read + write of every bucket record it touches (~1.3 ms at 2^26).
inline std::vector<uint64_t> host_chunk_cuts(uint64_t n, bool upload_bases, const HostKnobs& K) {
  std::vector<uint64_t> cuts{0};
  if (K.chunk_test) {
    for (uint64_t lo = K.chunk_test; lo < n; lo += K.chunk_test) cuts.push_back(lo);
  } else if (n >= 4 * HOST_CHUNK_MIN) {
    if (upload_bases) {
      // Bases travelling too (96 B per exponent): the link is the bottleneck and the kernels of a chunk finish long before the
      // next one has arrived; even chunks, small enough that the last one's kernels are a short tail behind the last byte.
      uint64_t k = (n + HOST_CHUNK_UPLOAD - 1) / HOST_CHUNK_UPLOAD;
      if (k < 2) k = 2;
      const uint64_t per = ((n + k - 1) / k + 31) & ~31ull;
      for (uint64_t lo = per; lo < n; lo += per) cuts.push_back(lo);
    } else {
      // Bases on the device: the kernels are the bottleneck (~1 G exponents/s against ~1.7 G/s of link).  Only the FIRST chunk's
      // upload is exposed, so it is small; each following chunk may be ~1.8 x the previous one and still arrive before the
      // kernels of its predecessor are done.
      uint64_t sz = n / 20 > HOST_CHUNK_MIN ? n / 20 : HOST_CHUNK_MIN;
      if (K.chunk_first_log) sz = 1ull << K.chunk_first_log;
      sz = (sz + 31) & ~31ull;
      uint64_t lo = 0;
      while (n - lo > sz + sz / 2) {  // the last chunk takes what is left, up to 1.5 x the next size
        lo += sz;
        cuts.push_back(lo);
        sz = ((uint64_t)((double)sz * K.chunk_growth) + 31) & ~31ull;
      }
    }
  }
  if (n) cuts.push_back(n);
  return cuts;
}

// The ranges a call of n independent items is dealt into over `devices` devices: as many as there are devices, fewer while a range would
// hold less than min_per_part items (cells of a multiexp: 32 exponents, batch_exp: 1024 points, the QAP matvec: 128 rows).
inline size_t range_parts(uint64_t n, size_t devices, uint64_t min_per_part) {
  size_t parts = devices;
  while (parts > 1 && n / parts < min_per_part) --parts;
  return parts;
}

// The cells of the single-process multi-GPU multiexp (host_entry.hip: msm_host_multi): pg contiguous POINT RANGES of the exponents before
// the first Eof -- cut[r] .. cut[r + 1], inner cuts at multiples of 32 so that density words are not shared -- x wg groups of scalar
// windows; empty ranges make no cell.  A cell runs on device `slot` of the call's device list and sees the slice [boff, boff + used) of
// the base vector: the bases its exponents consume.
struct HostCell {
  uint32_t slot = 0;
  uint64_t lo = 0, hi = 0;
  uint32_t wgi = 0;
  uint64_t boff = 0, used = 0;
};
struct CellPlan {
  uint32_t pg = 1, wg = 1;
  std::vector<uint64_t> cut;
  std::vector<HostCell> cells;
};
inline CellPlan plan_cells(const DensityPlan& P, uint64_t base_offset, size_t n_devices, const HostKnobs& K, const MsmKnobs& MK) {
  CellPlan C;
  const uint64_t n = P.live();
  uint32_t pg = (uint32_t)n_devices, wg = 1;
  if (K.plan_p && (size_t)K.plan_p * K.plan_w <= n_devices) { pg = K.plan_p; wg = K.plan_w; }  // (a plan the device set cannot hold: the default)
  if (wg > 1) {  // the window count of the range's geometry must divide (choose_geom takes care of that; W == 0: no such layout)
    const uint32_t W = choose_geom((n + pg - 1) / pg, 1, wg, MK).W;
    if (W == 0 || W % wg) wg = 1;
  }
  pg = (uint32_t)range_parts(n, pg, 32);
  // (the cuts are rounded UP to multiples of 32, which shortens the last range alone: fewer ranges while it would hold less than 32
  // exponents -- only calls of less than 63 exponents per range, which take MI355ZK_MULTI_MIN_LOG to get here)
  while (pg > 1 && n - (((n * (pg - 1) / pg) + 31) & ~31ull) < 32) --pg;
  C.pg = pg;
  C.wg = wg;
  C.cut.assign(pg + 1, 0);
  for (uint32_t r = 1; r < pg; ++r) C.cut[r] = ((n * r / pg) + 31) & ~31ull;
  C.cut[pg] = n;
  for (uint32_t r = 0; r < pg; ++r)
    for (uint32_t g = 0; g < wg; ++g) {
      if (C.cut[r + 1] <= C.cut[r]) continue;
      HostCell c;
      c.slot = (uint32_t)(C.cells.size() % n_devices);
      c.lo = C.cut[r];
      c.hi = C.cut[r + 1];
      c.wgi = g;
      // (the ranges end before the first exponent without a base -- the Eof is planned for the whole call -- so the slice holds every
      // base the cell asks for)
      c.boff = base_offset + P.rank(c.lo);
      c.used = P.rank(c.hi) - P.rank(c.lo);
      C.cells.push_back(c);
    }
  return C;
}

// The join of the cells' outcomes, with the rule shard.exchange defines.  rc[i]: cell i's return code, err[i]: its error index (relative
// to the cell's first exponent lo[i]; -1: none), eof_index: the Eof planned for the whole call (-1: none).  In cell order, the first
// device failure (rc < 0, or a code a cell cannot return: a cell never reports Eof, its range ends before the first exponent without a
// base) or non-canonical exponent WITHOUT an index ends the join; then a non-canonical exponent (bad arguments: the single-device call
// reports it before anything else too), then the Source errors by GLOBAL exponent index: the lowest identity, and the Eof last (every
// exponent before the Eof has a lower index).  index: what mi355zk_last_error_index reports (-1: nothing to report).
struct CellJoin {
  int rc = ZK_OK;
  long long index = -1;
};
inline CellJoin join_cells(const int* rc, const long long* err, const uint64_t* lo, size_t count, long long eof_index) {
  long long bad_idx = -1, ident_idx = -1;
  for (size_t i = 0; i < count; ++i) {
    if (rc[i] < 0) return {rc[i], -1};
    if (rc[i] == ZK_ERR_BAD_ARGS) {
      const long long g = err[i] >= 0 ? err[i] + (long long)lo[i] : -1;
      if (g < 0) return {ZK_ERR_BAD_ARGS, -1};
      if (bad_idx < 0 || g < bad_idx) bad_idx = g;
    } else if (rc[i] == ZK_ERR_UNEXPECTED_IDENTITY) {
      const long long g = err[i] + (long long)lo[i];
      if (ident_idx < 0 || g < ident_idx) ident_idx = g;
    } else if (rc[i] != ZK_OK) {
      return {ZK_ERR_DEVICE, -1};
    }
  }
  if (bad_idx >= 0) return {ZK_ERR_BAD_ARGS, bad_idx};
  if (ident_idx >= 0) return {ZK_ERR_UNEXPECTED_IDENTITY, ident_idx};
  if (eof_index >= 0) return {ZK_ERR_UNEXPECTED_EOF, eof_index};
  return {ZK_OK, -1};
}

// The row ranges of the QAP matvec over `parts` devices (host_ops.hip: sparse_matvec_host): cut[d] .. cut[d + 1], cuts of equal WEIGHT
// (rows + terms: a row costs a normalisation, a term an addition chain), found by one walk over row_ptr -- the variables of a circuit
// are far from equally used (the constant ONE sits in most constraints).  row_ptr[0 .. n_rows] as the caller gave it (not yet validated).
inline std::vector<size_t> weight_cuts(const uint32_t* row_ptr, size_t n_rows, size_t nnz, size_t parts) {
  std::vector<size_t> cut(parts + 1, n_rows);
  cut[0] = 0;
  const size_t weight = n_rows + nnz;
  size_t d = 1;
  for (size_t r = 0; r < n_rows && d < parts; ++r)
    while (d < parts && r + (size_t)row_ptr[r] >= weight * d / parts) cut[d++] = r;
  return cut;
}

// merge_pairs (host_ops.hip: dense_host) over ONE array seen at two offsets: power_pairs (utils.rs:133-135) is
// merge_pairs(v[0 .. n-1], v[1 .. n]), and uploading the array twice would double the PCIe traffic of a call the link already bounds -- a v2
// that starts `shift` (<= 16) records of `rec` bytes into v1 shares v1's upload.  Returns the shift, or (size_t)-1: separate uploads (or no v2).
// (the addresses are compared as integers -- the two pointers need not belong to one array -- and the vectors must really overlap:
// shift <= n; two separate short arrays that happen to sit within 16 records of each other are uploaded separately: ADVICE r4)
inline size_t shared_shift(const void* v1, const void* v2, size_t rec, size_t n) {
  const uintptr_t a1 = (uintptr_t)v1, a2 = (uintptr_t)v2;
  return (v2 && a2 >= a1 && (a2 - a1) % rec == 0 && (a2 - a1) / rec <= 16 && (a2 - a1) / rec <= n) ? (size_t)((a2 - a1) / rec) : (size_t)-1;
}

}  // namespace zk
