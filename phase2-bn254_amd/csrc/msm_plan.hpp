#pragma once
// The host-side PLAN of a multiexp (msm_host.hpp: msm_device): window geometry, reduce schedule, the partition plan of every chunk
// and the workspace layout -- pure arithmetic on the call's sizes and the knobs.  No HIP call and no getenv below msm_knobs(): the
// planner runs, and is tested, without a device (tests/test_msm_join_host.py).
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "host_util.hpp"
#include "msm_common.hpp"

namespace zk {

// Every environment knob of the multiexp's host side, read in ONE place (msm_knobs); the planner, the launch stages and the join take
// them as an argument.  Experiment / comparison switches unless noted; the defaults below are what an empty environment gives.
struct MsmKnobs {
  // read once per process
  int msm_c = 0;                  // MI355ZK_MSM_C: window bits 2..24 of a plain call (choose_geom)
  uint32_t radix_m = 0, radix_s = 0;  // MI355ZK_MSM_RADIX = "m,s": force B = m * 2^s (m odd, 3..15; s 2..22)
  bool radix_off = false;         //                     = "0": power-of-two layouts only
  int table_c = 0;                // MI355ZK_MSM_TABLE_C: window bits 4..24 of a table (table_window_bits)
  int part_lo = -1, part_st = 0;  // MI355ZK_PART_LO / MI355ZK_PART_ST: fine bits / super-tile size of the partition (choose_part)
  bool no_tail2d = false;         // MI355ZK_MSM_NO_TAIL2D: the levels-to-1024 reduce schedule
  bool no_small_scan = false;     // MI355ZK_MSM_NO_SMALL_SCAN: never the single-workgroup scan of short calls
  bool debug = false;             // MI355ZK_DEBUG: synchronise and report after every stage
  bool fused_a = false;           // MI355ZK_PART_FUSED_A: the one-kernel pass A, kept for the comparison in DESIGN.md
  uint32_t part_xcds = 8;         // MI355ZK_PART_XCDS: 1 disables the XCD-aware tile order
  bool acc_a4 = true;             // MI355ZK_ACC_NARROW unset: index lists walked four entries at a time
  int g1_pair = -1, g2_pair = -1; // MI355ZK_G1_PAIR / MI355ZK_G2_PAIR = 0 / 1: never / always a pair of lanes per bucket (-1: by size)
  int g2_waves = 0;               // MI355ZK_G2_WAVES = 1 / 2: always one / always two waves per SIMD (0: by what else runs)
  bool quad_tail = true;          // MI355ZK_MSM_QUAD = 0: no quad additions in the reduction
  uint32_t quad_max_chunks = 65536;  // MI355ZK_MSM_QUAD_MAX: the largest chunk count x windows of a level that runs four lanes per chunk
  bool trace_join = false;        // MI355ZK_TRACE_MSM: report the host join's time
  bool join_serial = false;       // MI355ZK_MSM_JOIN_SERIAL: never the helper threads
  // read per call
  uint32_t final_max = MSM_FINAL_MAX;  // MI355ZK_MSM_FINAL_MAX (>= 64): levels run while a window has more elements than this
  uint8_t logl[MSM_MAX_LEVELS] = {};   // MI355ZK_MSM_LOGL = "3,2,2": chunk length 2^k (k 1..5) of the first levels; 0: the schedule's own
  bool split_off = false;         // MI355ZK_MSM_SPLIT = 0: no quad-per-bucket launch for the long buckets of a short call
  uint32_t split_t = 0;           //                   = t: its threshold
};

inline MsmKnobs msm_knobs() {
  static const MsmKnobs process = [] {
    MsmKnobs K;
    auto num = [](const char* name, int unset) { const char* s = std::getenv(name); return s ? std::atoi(s) : unset; };
    auto set = [](const char* name) { return std::getenv(name) != nullptr; };
    K.msm_c = num("MI355ZK_MSM_C", 0);
    if (const char* s = std::getenv("MI355ZK_MSM_RADIX")) {
      int rm = 0, rs = 0;
      if (std::sscanf(s, "%d,%d", &rm, &rs) == 2 && rm >= 3 && rm <= 15 && (rm & 1) && rs >= 2 && rs <= 22) K.radix_m = (uint32_t)rm, K.radix_s = (uint32_t)rs;
      K.radix_off = s[0] == '0';
    }
    K.table_c = num("MI355ZK_MSM_TABLE_C", 0);
    K.part_lo = num("MI355ZK_PART_LO", -1);
    K.part_st = num("MI355ZK_PART_ST", 0);
    K.no_tail2d = set("MI355ZK_MSM_NO_TAIL2D");
    K.no_small_scan = set("MI355ZK_MSM_NO_SMALL_SCAN");
    K.debug = set("MI355ZK_DEBUG");
    K.fused_a = set("MI355ZK_PART_FUSED_A");
    K.part_xcds = num("MI355ZK_PART_XCDS", 0) >= 1 ? (uint32_t)num("MI355ZK_PART_XCDS", 0) : 8u;
    K.acc_a4 = !set("MI355ZK_ACC_NARROW");
    auto tri = [](const char* name) { const char* s = std::getenv(name); return !s ? -1 : s[0] == '0' ? 0 : 1; };
    K.g1_pair = tri("MI355ZK_G1_PAIR");
    K.g2_pair = tri("MI355ZK_G2_PAIR");
    if (const char* s = std::getenv("MI355ZK_G2_WAVES")) K.g2_waves = s[0] == '1' ? 1 : 2;
    if (const char* s = std::getenv("MI355ZK_MSM_QUAD")) K.quad_tail = s[0] != '0';
    if (const char* s = std::getenv("MI355ZK_MSM_QUAD_MAX")) K.quad_max_chunks = (uint32_t)std::atoi(s);
    K.trace_join = set("MI355ZK_TRACE_MSM");
    K.join_serial = set("MI355ZK_MSM_JOIN_SERIAL");
    return K;
  }();
  MsmKnobs K = process;
  if (const char* s = std::getenv("MI355ZK_MSM_FINAL_MAX"))
    if (std::atoi(s) >= 64) K.final_max = (uint32_t)std::atoi(s);
  if (const char* s = std::getenv("MI355ZK_MSM_LOGL")) {
    // field k of the comma-separated list, its first character: the chunk length of level k
    for (uint32_t lv = 0; lv < MSM_MAX_LEVELS; ++lv) {
      uint32_t k = 0;
      const char* q = s;
      while (k < lv && *q) { if (*q == ',') ++k; ++q; }
      if (k == lv && *q >= '1' && *q <= '5') K.logl[lv] = (uint8_t)(*q - '0');
    }
  }
  if (const char* s = std::getenv("MI355ZK_MSM_SPLIT")) {
    K.split_off = s[0] == '0' && s[1] == 0;
    if (std::atoi(s) > 0) K.split_t = (uint32_t)std::atoi(s);
  }
  return K;
}

inline size_t align_up(size_t x, size_t a = 256) { return (x + a - 1) / a * a; }

// Window size.  The reference uses c = ceil(ln n) (multiexp.rs:341-345), sized for its
// one-thread-per-window scan.  Here every bucket of every window is a lane, so c trades
// W*n mixed adds (10 mul each) against W*2^(c-1) buckets to reduce (~35 mul each) while keeping
// enough buckets to fill 256 CUs.  Override: env MI355ZK_MSM_C (MsmKnobs::msm_c).
// widths for a maximum window size c: top window c-1 bits (unsigned), the rest as even as possible, all <= c
inline MsmGeom make_geom(uint32_t c) {
  MsmGeom G{};
  G.rmul = 1;
  G.c = c;
  uint32_t W = 1;
  while ((W - 1) * c + (c - 1) < 254) ++W;      // smallest W with (W-1) windows of <= c bits + a top window of <= c-1 bits
  G.W = W;
  G.nb = 1u << (c - 1);
  uint32_t top = c - 1;
  if (W == 1) top = 254 < top ? 254 : top;
  uint32_t rest = 254 > top ? 254 - top : 0;    // bits for windows 0..W-2
  uint32_t base = W > 1 ? rest / (W - 1) : 0, rem = W > 1 ? rest % (W - 1) : 0;
  uint32_t bit = 0;
  for (uint32_t w = 0; w + 1 < W; ++w) {
    G.width[w] = (uint8_t)(base + (w < rem ? 1 : 0));
    G.shift[w] = (uint8_t)bit;
    bit += G.width[w];
  }
  G.width[W - 1] = (uint8_t)(254 - bit);        // == top when rest was spread exactly (always: base*(W-1)+rem == rest)
  G.shift[W - 1] = (uint8_t)bit;
  return G;
}

// mixed-radix layout: B = rmul * 2^rshift, nb = B/2, the smallest W with B^(W-1) * nb >= 2^254 (scalars are < r < 2^254)
inline MsmGeom make_geom_radix(uint32_t rmul, uint32_t rshift) {
  MsmGeom G{};
  G.rmul = rmul;
  G.rshift = rshift;
  const double B = std::ldexp((double)rmul, (int)rshift);
  G.nb = (rmul << rshift) / 2;
  G.c = 1;
  while ((1u << G.c) <= G.nb) ++G.c;           // field values 0..nb
  uint32_t W = 2;
  while ((W - 1) * std::log2(B) + std::log2((double)G.nb) < 254.001) ++W;
  G.W = W;
  return G;
}

// top_values: the number of digit values the TOP window can take (2^254 / B^(W-1), or 2^width): a layout whose top window is
// much narrower than the others sends n / top_values points into each of its buckets.
inline double geom_cost(double W, double nbk, double field_bits, uint64_t n, double top_values) {
  // per (point, window): one mixed add (10 units) + one radix-sort pass per 8 key bits (0.7 units each,
  // measured); per bucket: ~45 units of reduction
  double cost = W * ((10.0 + 0.7 * std::ceil(field_bits / 8.0)) * (double)n + 45.0 * nbk);
  // occupancy term: fewer than ~2^17 bucket lanes leaves CUs idle during accumulation
  double lanes = W * nbk;
  if (lanes < 131072.0) cost *= (1.0 + 0.5 * (131072.0 / lanes - 1.0));
  // A top window whose buckets pass the heavy threshold (msm_device: max(64, 2 * mean + 16) for a short call) takes the
  // segment-parallel path IN FRONT of the accumulation: ~0.18 ms of a 1-ms call at 2^16 points (B = 13 * 2^10: 169 top values, 388
  // points per top bucket: profiles/r03_msm16_timeline.txt).  A constant the size of that detour: decisive for short calls, nothing
  // at 2^20 and beyond (where the segments also run at throughput).
  // Below that threshold a lane still walks the top bucket alone, ~8 us per point whatever the rest of the launch does (2^15
  // points, B = 3 * 2^12: 46 points per top bucket among buckets of 5: the launch lasts 0.44 ms instead of 0.2): ~5e5 units per
  // point a top bucket holds beyond what the ordinary buckets' tail reaches anyway.
  const double mean = (double)n / nbk;
  const double heavy = std::max(64.0, 2.0 * mean + 16.0);
  const double top_len = (double)n / top_values;
  if (top_len > heavy) cost += 1.2e7;
  else if (top_len > 2.0 * mean + 16.0) cost += (top_len - (2.0 * mean + 16.0)) * 5e5;
  return cost;
}

inline MsmGeom choose_geom(uint64_t n, int group, uint32_t wgroups, const MsmKnobs& K) {
  if (K.radix_m && wgroups == 1) return make_geom_radix(K.radix_m, K.radix_s);
  if (K.msm_c >= 2 && K.msm_c <= 24 && wgroups == 1) return make_geom((uint32_t)K.msm_c);
  // Short calls (n < 2^20, all windows on one GPU): MEASURED choice.  The launch no longer fills the device there and the model
  // below -- throughput of additions, 45 units per bucket -- misses what a call costs: the reduce is a chain of dependent additions
  // whose length depends on c alone (c = 10: 0.12 ms ... 16: 0.40, 17: 0.62) and the accumulation reaches its throughput only from
  // ~2^19 bucket lanes on.  profiles/r03_small_n_window_sweep.txt: every c at every size; the table is its minimum (8 - 15 % per call
  // against the model's choice; power-of-two windows, whose top window is as wide as the others).
  if (wgroups == 1 && n < (1ull << 20)) {
    uint32_t lg = 0;
    while ((1ull << lg) < n) ++lg;
    uint32_t c = lg <= 10 ? 10u : lg <= 12 ? 11u : lg == 13 ? 12u : lg <= 15 ? 13u : lg <= 17 ? 15u : 16u;
    // G2 (profiles/r03_small_n_window_sweep.txt, second half): an addition costs three times G1's and so does every step of the
    // reduce chain -- one bit narrower between 2^14 and 2^18 (2^14: 1.43 -> 1.33 ms, 2^16: 1.71 -> 1.61, 2^18: 2.54 -> 2.49)
    if (group == 2) c = lg <= 10 ? 10u : lg == 11 ? 11u : lg <= 15 ? 12u : lg <= 17 ? 14u : lg == 18 ? 15u : 16u;
    // (end of round 4, with the pair-per-bucket accumulation: profiles/r04_small_n_sweep_pair.txt -- G1 2^15: c = 15 -> 13, 0.475 -> 0.45 ms;
    // G2 2^15: 14 -> 12, 1.08 -> 0.99 ms; G2 2^17: 15 -> 14, 1.52 -> 1.46 ms; every other entry stayed the minimum)
    return make_geom(c);
  }
  // wgroups > 1: the windows are dealt out to that many ranks, so W must divide evenly (per-rank cost ~ total / wgroups)
  uint32_t best_c = 0;
  double best = 1e300;
  for (uint32_t c = 4; c <= 24; ++c) {
    double W = std::ceil((254.0 + 1.0) / c);  // (W-1)*c + (c-1) >= 254
    if ((uint32_t)W % wgroups) continue;
    // (make_geom: the top window keeps what the W - 1 equal windows leave of the 254 bits, at most c - 1)
    const MsmGeom Gc = make_geom(c);
    double cost = geom_cost(W, std::ldexp(1.0, (int)c - 1), c, n, std::ldexp(1.0, (int)Gc.width[Gc.W - 1]));
    if (cost < best) { best = cost; best_c = c; }
  }
  MsmGeom G{};
  if (best_c) G = make_geom(best_c);
  if (K.radix_off && best_c) return G;
  // a mixed-radix layout must win by 1.5 % to be taken (its host join is slightly longer)
  for (uint32_t rmul = 3; rmul <= 15; rmul += 2)
    for (uint32_t rshift = 4; rshift <= 22; ++rshift) {
      MsmGeom R = make_geom_radix(rmul, rshift);
      if (R.W > 64 || R.c > 24 || R.W % wgroups) continue;
      const double top_values = std::exp2(254.0 - (R.W - 1.0) * std::log2(std::ldexp((double)rmul, (int)rshift)));
      double cost = geom_cost(R.W, R.nb, R.c, n, top_values);
      if (cost < 0.985 * best) { best = cost / 0.985; G = R; }
    }
  return G;
}

// Window width of a TABLE-MODE call (msm_device, table_stride != 0) over a base vector of n_bases points: one bucket set serves all
// windows, so the reduction is paid once and the window may be wider than choose_geom's (fewer windows = fewer additions); what
// limits it is the length of the one reduce chain and the bucket lists getting short.  Measured (profiles/r03_table_mode.txt);
// override: env MI355ZK_MSM_TABLE_C (MsmKnobs::table_c).  Power-of-two windows only: table[w] = 2^shift_w * P.
inline uint32_t table_window_bits(uint64_t n_bases, int group, const MsmKnobs& K) {
  if (K.table_c >= 4 && K.table_c <= 24) return (uint32_t)K.table_c;
  uint32_t lg = 0;
  while ((1ull << lg) < n_bases) ++lg;
  // Only the smallest c of every window count matters (17: 15 windows, 19: 14, 20: 13, 22: 12, 24: 11).  Every bucket of the one set
  // is populated (the top window's unsigned digits reach all of them), so the reduce runs at its full length: c = 22 costs 1.0 ms,
  // 23: 1.6, 24: 2.8.  Short vectors need bucket LANES before anything else (2^16 points at the plain call's c = 15: 16 k lanes, 1.18 ms
  // against 0.72 at c = 17) -- and gain nothing over the plain call below 2^19.
  if (group == 2) return lg <= 18 ? 17u : lg == 19 ? 19u : 20u;   // (a G2 reduce step costs three G1 steps: 15 - 25 % over the plain call from 2^16 on)
  return lg <= 16 ? 17u : lg <= 22 ? 20u : 22u;
}

// partition geometry for n scalars, WL windows of nb bucket slots each
inline PartGeom choose_part(uint64_t n, uint32_t WL, uint32_t nb, const MsmKnobs& K) {
  PartGeom P{};
  uint32_t lo_cap = 0;
  while ((1u << lo_cap) < nb && lo_cap < PART_LO_MAX) ++lo_cap;  // one bin holds everything, or 2^PART_LO_MAX buckets
  auto nbin_of = [&](uint32_t lo) { return (uint32_t)(((uint64_t)nb + (1ull << lo) - 1) >> lo); };
  // as fine as the pass-A histogram (WL * nbin words of LDS) allows, but no finer than ~8192 elements per bin need
  // pass A keeps WL * nbin 16-bit counters in LDS (two workgroups per CU while they fit PART_LDS_A, one up to twice that);
  // pass B scans nbin words with 1024 lanes x 4
  auto fits_lds = [&](uint32_t lo, uint64_t budget) { return (uint64_t)WL * nbin_of(lo) * 2 <= budget && nbin_of(lo) <= 4 * PART_THREADS; };
  auto fits = [&](uint32_t lo) { return fits_lds(lo, 2 * PART_LDS_A); };
  auto pop = [&](uint32_t lo) { return (uint64_t)n * (1ull << lo) / nb; };  // mean elements per (window, bin)
  uint32_t lo = lo_cap;
  const uint64_t pop_target = 12288;
  const uint64_t pop_cap = (uint64_t)PART_EC * PART_THREADS * 85 / 100;     // pass C holds a bin in registers: stay clear of the cliff
  while (lo > 0 && pop(lo) > pop_target && fits_lds(lo - 1, PART_LDS_A)) --lo;
  while (lo > 0 && pop(lo) > pop_cap && fits(lo - 1)) --lo;
  while (!fits(lo) && lo < PART_LO_MAX) ++lo;
  if (K.part_lo >= 0 && K.part_lo <= (int)lo_cap && fits((uint32_t)K.part_lo)) lo = (uint32_t)K.part_lo;
  P.lo_bits = lo;
  P.nbin = nbin_of(lo);
  // Super-tiles as large as LDS allows: a pass-B workgroup pays its scans and barriers once, whatever it moves (2^20 exponents, 16
  // windows: 0.150 ms with 2048-element tiles, 0.049 ms with 16384; round 2 shrank the tiles until there were 512 of them PER WINDOW,
  // which at 16 windows is 8192 workgroups of two elements per lane).  Smaller only while a launch would not even give every CU one
  // workgroup (n_st * WL < 256: 2^16 exponents run 4096-element tiles).
  uint32_t st = PART_MAX_ST;
  while (st > PART_THREADS && (n / st) * WL < 256) st >>= 1;
  if (K.part_st >= (int)PART_THREADS && K.part_st <= (int)PART_MAX_ST && K.part_st % (int)PART_THREADS == 0) st = (uint32_t)K.part_st;
  // pass B holds the tile (8 B per element) and nbin words in LDS
  while (st > PART_THREADS && (uint64_t)st * 8 + (uint64_t)P.nbin * 8 + 256 > PART_LDS_MAX) st -= PART_THREADS;
  if ((uint64_t)st * 8 + (uint64_t)P.nbin * 8 + 256 > PART_LDS_MAX) st = 0;  // cannot happen: nbin <= 4096
  P.st = st;
  P.n_st = (uint32_t)((n + st - 1) / st);
  P.rows_per_chunk = P.n_st > 64 ? (P.n_st + 63) / 64 : 1;
  P.n_chunk = (P.n_st + P.rows_per_chunk - 1) / P.rows_per_chunk;
  return P;
}

// ---- the plan of one call

struct MsmRequest {
  int group = 1;                    // 1: G1, 2: G2 (record sizes; the measured choices differ)
  uint64_t n = 0;                   // exponents (> 0)
  uint64_t base_offset = 0;
  uint32_t wgroups = 1, wgroup = 0; // only window group `wgroup` of `wgroups` equal groups is evaluated
  uint32_t n_chunks = 1;            // a streamed call: exponents [cuts[c], cuts[c+1]) per chunk; cuts == nullptr: one chunk, the whole call
  const uint64_t* cuts = nullptr;
  bool two_sets = false;            // a second base vector under the same exponents
  uint64_t table_stride = 0;        // != 0: table mode, windows of make_geom(table_c)
  uint32_t table_c = 0;
  uint32_t n_vectors = 1;           // > 1: a BATCH -- that many exponent vectors of n exponents each over the one base vector (one pipeline pass)
};

// per chunk: its partition geometry, and what one lane may walk before its bucket counts as heavy
struct ChunkPlan {
  uint64_t lo, n, m, np;  // np: length of the array the partition sees (table mode: all key planes as one)
  PartGeom P;
  uint32_t ncell, heavy, heavy_seg, hb, max_items;
  bool small_scan;              // short calls: the four column scans + the big-bin plan in one single-workgroup launch
  uint32_t split_t, split_hb;   // short calls: buckets longer than split_t take the quad-per-bucket launch (0: none)
};

// byte offsets into the call's workspace, in this order, each a multiple of 256
struct MsmLayout {
  // the window-major keys of pass A are dead once pass B has run; pass C writes the index lists over them
  size_t keys, pairs, tile_hist, tile_off, csum, total, bin_start, out_start;
  // big bins (msm_bigbin_*): per-bucket counts and cursors (contiguous: one memset), the list of big bins, the plan
  size_t gcnt, gcur, big_col, big_seg, big_plan;
  size_t first, last, hist, sizes_b, ids_b, item_off, seg_sums, buckets, partA, partS;
  size_t rc;      // 2-D tail: row sums, then column sums, per window
  size_t wsums;
  size_t err;     // [0] lowest identity base index, [1] lowest index of a non-canonical exponent -- right behind the window sums: ONE copy brings both back
  size_t sumtmp;  // slice sums of msm_tree_kernel (two ping-pong halves): n_out jobs per window, slices of the longest job
  size_t total_bytes;
  size_t back_bytes() const { return (err - wsums) + 16; }  // the window sums, their alignment padding, the two error words
};

struct MsmPlan {
  int rc = ZK_OK;               // ZK_ERR_BAD_ARGS: the call is refused, nothing else is valid
  int group = 1;
  bool tmode = false;           // table mode: ONE bucket set serves all windows
  uint32_t n_vectors = 1;       // a batch: WL = n_vectors * WD bucket sets, vector v owns sets [v * WD, (v + 1) * WD)
  MsmGeom G{};
  uint32_t WD = 0, w_lo = 0, w_hi = 0;  // this call's windows (digit planes)
  uint32_t WL = 0;              // bucket sets: one per window (and per vector of a batch), or ONE in table mode
  uint32_t n_buckets = 0;
  uint64_t m_max = 0;
  // reduction: running-sum levels (msm_reduce_level_kernel, chunk length 2^lvl_logl) while more than final_max elements per window are
  // left, then the bit-decomposition stage (msm_tree_kernel), with or without the 2-D tail
  uint32_t n_levels = 0, lvl_cnt[MSM_MAX_LEVELS + 1] = {}, lvl_chunks[MSM_MAX_LEVELS + 1] = {}, lvl_logl[MSM_MAX_LEVELS + 1] = {};
  uint64_t total_chunks = 1;
  uint32_t final_cnt = 0;
  uint32_t final_off = 0;       // bucket x of a window has weight x + 1; chunk sums have weight ch
  bool tail2d = false;
  uint32_t cols_log = 0, t_cols = 0, t_rows = 0;
  uint32_t final_bits = 1;      // bits of the column index (of the whole index without the 2-D tail)
  uint32_t row_bits = 0;        // bits of the row index
  // per window n_out partial sums come back: one A-sum per level, then one sum per (column) bit, then one per row bit; partial sum k
  // carries the power of two 2^e_k[k] inside its window
  uint32_t n_out = 0, e_k[MSM_MAX_JOBS] = {}, e_max = 0;
  uint32_t tree_cnt = 0;
  uint64_t tree_tmp = 0;
  std::vector<ChunkPlan> chunks;
  MsmLayout L{};
};

inline int msm_plan_fill(const MsmRequest& R, const MsmKnobs& K, MsmPlan& P) {
  const uint64_t n = R.n;
  const bool g1 = R.group == 1;
  const size_t rec_bytes = g1 ? 128 : 256;  // sizeof(XYZZ<F>)
  P.group = R.group;
  if (R.wgroups == 0 || R.wgroup >= R.wgroups) return ZK_ERR_BAD_ARGS;
  const bool tmode = P.tmode = R.table_stride != 0;
  if (tmode && (R.wgroups != 1 || R.n_chunks != 1 || R.two_sets || R.table_c < 4 || R.table_c > 24 || R.base_offset > R.table_stride)) return ZK_ERR_BAD_ARGS;
  const uint32_t B = P.n_vectors = R.n_vectors;
  if (B == 0) return ZK_ERR_BAD_ARGS;
  if (B > 1 && (tmode || R.n_chunks != 1 || R.cuts != nullptr || R.two_sets || R.wgroups != 1)) return ZK_ERR_BAD_ARGS;
  const uint64_t whole[2] = {0, n};
  const uint32_t n_chunks = R.n_chunks;
  const uint64_t* cuts = R.cuts ? R.cuts : whole;
  // (cuts == nullptr with more than one chunk: not one of msm_device's checks -- it fills both from MsmChunks -- but a request can be built that way)
  if (n_chunks == 0 || (R.cuts == nullptr && n_chunks != 1) || cuts[0] != 0 || cuts[n_chunks] != n) return ZK_ERR_BAD_ARGS;
  if (n_chunks > 1 && R.two_sets) return ZK_ERR_BAD_ARGS;
  uint64_t n_max = 0;
  for (uint32_t c = 0; c < n_chunks; ++c) {
    if (cuts[c + 1] <= cuts[c] || (c > 0 && (cuts[c] & 31))) return ZK_ERR_BAD_ARGS;  // (density words are not shared between chunks)
    if (cuts[c + 1] - cuts[c] > n_max) n_max = cuts[c + 1] - cuts[c];
  }
  const MsmGeom G = P.G = tmode ? make_geom(R.table_c) : choose_geom(n, R.group, R.wgroups, K);
  if (G.W == 0 || G.W % R.wgroups) return ZK_ERR_BAD_ARGS;
  const uint32_t WD = P.WD = G.W / R.wgroups;
  P.w_lo = R.wgroup * WD;
  P.w_hi = P.w_lo + WD;
  // (a batch: the geometry above is that of ONE vector of n exponents; the vectors only multiply the bucket sets)
  if (B > 1 && (uint64_t)B * WD > MSM_BATCH_MAX_WINDOWS) return ZK_ERR_BAD_ARGS;
  const uint32_t WL = P.WL = tmode ? 1u : B * WD;
  if (tmode && (uint64_t)G.W * R.table_stride > 0x7fffffffull) return ZK_ERR_BAD_ARGS;  // (an index-list entry is a 31-bit base index + sign)
  const uint64_t m_max = P.m_max = tmode ? ((n_max + 3) & ~3ull) * WD : n_max * WL;
  if (m_max > 0xfffffff0ull) return ZK_ERR_BAD_ARGS;  // pair positions are u32
  // bucket ids are u32 (a single call: W * nb <= 64 * 2^23), and a pair of lanes per bucket counts 2 * n_buckets threads in u32
  if ((uint64_t)WL * G.nb > (B > 1 ? 0x7ffffff0ull : 0xfffffff0ull)) return ZK_ERR_BAD_ARGS;
  const uint32_t n_buckets = P.n_buckets = WL * G.nb;
  // chunk length per level: 2L serial additions per lane, so shorter chunks once lanes are scarce
  uint32_t final_cnt = G.nb, n_levels = 0;
  // 2-D TAIL (round 3): once at most 2^17 elements are left over all windows (and at most 2^18 per window), the weighted sum of the
  // last array S is finished in TWO tree launches instead of further levels and a bit decomposition of what they leave:
  //   x = r * cols + c:   sum_x (x + off) S[x] = cols * sum_r r R_r + sum_c (c + off) C_c,   R_r / C_c = the row / column sums,
  // launch 1 = the rows, the columns (<= 512 elements each) and the levels' A[] as plain tree sums, launch 2 = the bit decompositions of
  // R and C (and the A[] slice sums).  A running-sum level costs 2L dependent additions and a launch however few lanes it has left;
  // the tail is a chain: table mode (ONE window of 2^19 buckets) 0.545 -> 0.424 ms at 2^20.
  // MsmKnobs::no_tail2d restores the levels-to-1024 schedule for the comparison.
  // (rows and columns of at least 128 elements: a tree workgroup spends nine rounds on its slice however few elements it holds, so
  // 16 windows x 8192 elements as 64 x 128 made the 2^20 reduce SLOWER, 0.40 -> 0.71 ms; G1 only: a G2 tree round costs three G1
  // rounds and the two launches gained nothing over the levels, 1.36 -> 1.38 ms)
  auto tail_fits = [&](uint32_t cnt) { return !K.no_tail2d && g1 && (uint64_t)cnt * WL <= (1ull << 17) && cnt >= (1u << 15) && cnt <= (1u << 18); };
  while (final_cnt > K.final_max && n_levels < MSM_MAX_LEVELS) {
    if (tail_fits(final_cnt)) break;
    uint32_t logl = (uint64_t)final_cnt * WL >= (1ull << 20) ? 3 : 2;
    if (K.logl[n_levels]) logl = K.logl[n_levels];   // (experiments: the forced chunk length 2^k of the first levels)
    P.lvl_cnt[n_levels] = final_cnt;
    P.lvl_logl[n_levels] = logl;
    P.lvl_chunks[n_levels] = (final_cnt + (1u << logl) - 1) >> logl;
    P.total_chunks += P.lvl_chunks[n_levels];
    final_cnt = P.lvl_chunks[n_levels];
    ++n_levels;
  }
  P.n_levels = n_levels;
  P.final_cnt = final_cnt;
  const uint32_t final_off = P.final_off = n_levels == 0 ? 1u : 0u;
  const bool tail2d = P.tail2d = tail_fits(final_cnt);
  if (tail2d) {
    uint32_t lg = 0;
    while ((1u << lg) < final_cnt) ++lg;
    P.cols_log = (lg + 1) / 2;
  }
  const uint32_t t_cols = P.t_cols = tail2d ? 1u << P.cols_log : final_cnt, t_rows = P.t_rows = tail2d ? (final_cnt + t_cols - 1) / t_cols : 0;
  while ((1u << P.final_bits) <= t_cols - 1 + final_off) ++P.final_bits;
  while (t_rows > 1 && (1u << P.row_bits) <= t_rows - 1) ++P.row_bits;

  P.chunks.resize(n_chunks);
  uint64_t keys_cap = 0, tile_hist_b = 0, tile_off_b = 0, csum_b = 0;
  uint32_t ncell_max = 0, hb_max = 0, items_max = 0;
  for (uint32_t c = 0; c < n_chunks; ++c) {
    ChunkPlan& C = P.chunks[c];
    C.lo = cuts[c];
    C.n = cuts[c + 1] - cuts[c];
    C.np = tmode ? ((C.n + 3) & ~3ull) * WD : C.n;
    C.m = C.np * WL;
    C.P = choose_part(C.np, WL, G.nb, K);
    if (C.P.st == 0) return ZK_ERR_BAD_ARGS;
    // a batch never leaves choose_part with a histogram its budget does not hold (one call's W <= 64 windows always fit at lo = PART_LO_MAX)
    if (B > 1 && (uint64_t)WL * C.P.nbin * 2 > 2ull * PART_LDS_A) return ZK_ERR_BAD_ARGS;
    C.ncell = WL * C.P.nbin;
    C.small_scan = !K.no_small_scan && (uint64_t)C.P.n_st * C.ncell <= (1u << 16);
    // index lists: every bucket start is padded to a multiple of 4 entries (<= 3 per bucket), every bin region to 4
    const uint64_t vals_cap = C.m + 3ull * n_buckets + 4ull * C.ncell + 4;
    if (vals_cap > 0xfffffff0ull) return ZK_ERR_BAD_ARGS;
    keys_cap = std::max(keys_cap, vals_cap);
    tile_hist_b = std::max<uint64_t>(tile_hist_b, (uint64_t)C.P.n_st * ((C.ncell + 1) & ~1u) * 2);
    tile_off_b = std::max<uint64_t>(tile_off_b, (uint64_t)C.P.n_st * C.ncell * 4);
    csum_b = std::max<uint64_t>(csum_b, (uint64_t)C.P.n_chunk * C.ncell * 4);
    ncell_max = std::max(ncell_max, C.ncell);
    // a bucket is "heavy" when it is far longer than the mean; at most m / heavy buckets can be
    // ... and, more to the point, when ONE lane walking it would outlast the whole launch: the lanes of a launch share ~2^18 lane
    // slots (256 CUs x 4 SIMDs x 4 waves x 64), so a launch lasts about m / 2^18 additions per slot; a longer bucket is a straggler
    // (it starts first -- buckets run in size order -- but finishes alone).  Prover-like exponents produce such buckets by the
    // hundred (every byte-sized witness value lands in one of 255 buckets of window 0).
    // Short calls are latency-bound instead: a lane adds a point to its bucket every ~8 us whatever else the device does (ten
    // dependent field products), so a bucket of 100 entries among buckets of 6 holds the launch for 0.8 ms (measured at 2^18
    // prover-like exponents: the 255 byte-valued buckets of window 0).  Hence a floor of 64, a margin of 16 over twice the mean,
    // and segments short enough (heavy_seg) that a segment's 64 lanes add a handful of points each before the tree.
    const uint64_t mean_len = C.m / n_buckets + 1;
    uint64_t heavy64 = mean_len * 8 + 1024;
    const uint64_t heavy_cap = (C.m >> 17) > 64 ? (C.m >> 17) : 64;  // 8 us per entry against ~2^-17 x m x 8 us for the launch at full throughput
    if (heavy64 > heavy_cap) heavy64 = heavy_cap;
    if (heavy64 < 2 * mean_len + 16) heavy64 = 2 * mean_len + 16;   // never the ordinary buckets
    C.heavy = (uint32_t)(heavy64 > 0xffffffffull ? 0xffffffffull : heavy64);
    C.heavy_seg = 128;
    while (C.heavy_seg < MSM_HEAVY_SEG && ((uint64_t)C.heavy_seg << 14) < C.m) C.heavy_seg <<= 1;
    C.hb = n_buckets < MSM_HEAVY_BLOCKS ? n_buckets : MSM_HEAVY_BLOCKS;
    if ((uint64_t)C.hb > C.m / C.heavy + 1) C.hb = (uint32_t)(C.m / C.heavy + 1);
    C.max_items = (uint32_t)(C.m / C.heavy_seg) + C.hb;  // every heavy bucket adds at most one partial segment
    hb_max = std::max(hb_max, C.hb);
    items_max = std::max(items_max, C.max_items);
    // Quad-per-bucket launch for the long buckets of a SHORT, unchunked call (msm_accumulate_split_kernel): while the lane-per-bucket
    // launch fits the device about once (<= 2^18 bucket lanes), its duration is its longest bucket.  Threshold: the mean length plus
    // one standard deviation of a Poisson count (~10 % of the buckets of uniform exponents), at least 4 (a lane per entry of a quad).
    // The two launches run one after the other (same stream): what is gained is the difference between the long buckets' chains.
    // MsmKnobs::split_off disables, split_t forces the threshold.
    // (measured, tools/ab_split.sh: G1 2^10 .. 2^14 points -4 .. -9 % per call, nothing at 2^15 .. 2^17, +3 .. 5 % from 2^18 on; G2: -2 % at 2^12, +2 % at 2^16)
    C.split_t = 0;
    C.split_hb = 0;
    if (!K.split_off && n_chunks == 1 && n_buckets <= (g1 ? 1u << 18 : 1u << 16) && !tmode) {
      const double mean = (double)C.m / n_buckets;
      uint32_t t = (uint32_t)std::ceil(mean + std::sqrt(mean + 1.0));
      if (K.split_t) t = K.split_t;
      if (t < 4) t = 4;
      if (t < C.heavy) {
        C.split_t = t;
        const uint64_t cap = C.m / (t + 1) + 1;    // buckets longer than t
        C.split_hb = (uint32_t)(cap < n_buckets ? cap : n_buckets);
      }
    }
  }
  P.n_out = n_levels + P.final_bits + P.row_bits;
  if (P.n_out + 2 > MSM_MAX_JOBS) return ZK_ERR_BAD_ARGS;
  // P[w][k] carries 2^e_k: a level's A-sums the product of the chunk lengths below it, the bits of the last array theirs on top
  uint32_t e_lv = 0;
  for (uint32_t lv = 0; lv < n_levels; ++lv) {
    P.e_k[lv] = e_lv;
    e_lv += P.lvl_logl[lv];
  }
  for (uint32_t j = 0; j < P.final_bits; ++j) P.e_k[n_levels + j] = e_lv + j;
  for (uint32_t j = 0; j < P.row_bits; ++j) P.e_k[n_levels + P.final_bits + j] = e_lv + P.cols_log + j;   // (2-D tail: the row index weighs cols = 2^cols_log)
  for (uint32_t k = 0; k < P.n_out; ++k) P.e_max = std::max(P.e_max, P.e_k[k]);
  P.tree_cnt = n_levels ? P.lvl_chunks[0] : final_cnt;
  P.tree_tmp = (uint64_t)P.n_out * ((P.tree_cnt + MSM_TREE_SLICE - 1) / MSM_TREE_SLICE);
  // the grid of a tree launch is (blocks per window) x WL: at most n_out + 2 jobs of at most max(slices of the longest job, rows, columns) blocks
  if (B > 1 && (uint64_t)(P.n_out + 2) * std::max<uint64_t>((P.tree_cnt + MSM_TREE_SLICE - 1) / MSM_TREE_SLICE, std::max(t_rows, t_cols)) * WL > 0x7fffffffull)
    return ZK_ERR_BAD_ARGS;

  MsmLayout& L = P.L;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes); return o; };
  L.keys = take((size_t)keys_cap * 4), L.pairs = take((size_t)m_max * 8);
  L.tile_hist = take((size_t)tile_hist_b), L.tile_off = take((size_t)tile_off_b);
  L.csum = take((size_t)csum_b), L.total = take((size_t)ncell_max * 4);
  L.bin_start = take((size_t)(ncell_max + 1) * 4), L.out_start = take((size_t)(ncell_max + 1) * 4);
  L.gcnt = take((size_t)n_buckets * 4), L.gcur = take((size_t)n_buckets * 4);
  L.big_col = take((size_t)ncell_max * 4), L.big_seg = take((size_t)ncell_max * 4), L.big_plan = take(sizeof(BigPlan));
  L.first = take((size_t)(n_buckets + 1) * 4), L.last = take((size_t)(n_buckets + 1) * 4), L.hist = take(MSM_SIZE_BINS * 4);
  L.sizes_b = take((size_t)n_buckets * 4), L.ids_b = take((size_t)n_buckets * 4);
  L.item_off = take((size_t)(hb_max + 2) * 4);
  L.seg_sums = take((size_t)items_max * rec_bytes);
  L.buckets = take((size_t)n_buckets * rec_bytes);
  L.partA = take((size_t)WL * P.total_chunks * rec_bytes);
  L.partS = take((size_t)WL * P.total_chunks * rec_bytes);
  L.rc = take((size_t)WL * (t_rows + t_cols) * rec_bytes);
  L.wsums = take((size_t)WL * P.n_out * rec_bytes);
  L.err = take(16);
  L.sumtmp = take((size_t)WL * P.tree_tmp * 2 * rec_bytes);
  L.total_bytes = off;
  return ZK_OK;
}

inline MsmPlan msm_plan(const MsmRequest& R, const MsmKnobs& K) {
  MsmPlan P;
  P.rc = msm_plan_fill(R, K, P);
  return P;
}

// ---- a batch (MsmRequest::n_vectors): how it is cut into pipeline passes; the limits are msm_common.hpp's MSM_BATCH_*
// vectors per pipeline pass of a batch of B vectors of n exponents (G = choose_geom(n, group, 1, K)): the most those limits and msm_plan_fill allow, at
// most B; 1 = no pass is worth its name (the caller runs single calls).  A batch runs ceil(B / split) passes over consecutive vectors.
inline uint32_t msm_batch_split(uint64_t n, uint32_t B, const MsmGeom& G, int group, const MsmKnobs& K) {
  if (B <= 1 || n == 0 || G.W == 0) return B ? 1u : 0u;
  uint32_t per = std::min<uint32_t>(B, MSM_BATCH_MAX_WINDOWS / G.W);
  while (per > 1) {
    MsmRequest R;
    R.group = group;
    R.n = n;
    R.n_vectors = per;
    const MsmPlan P = msm_plan(R, K);
    if (P.rc == ZK_OK && P.L.total_bytes <= MSM_BATCH_WS_MAX) break;
    // the workspace is (nearly) linear in the vectors: aim at the budget, and always move
    uint64_t next = per - 1;
    if (P.rc == ZK_OK) next = std::min<uint64_t>(next, (uint64_t)((double)per * (double)MSM_BATCH_WS_MAX / (double)P.L.total_bytes));
    else next = std::min<uint64_t>(next, per - per / 8);
    per = (uint32_t)std::max<uint64_t>(next, 1);
  }
  return per;
}
// pass p of the ceil(B / per) passes: `count` consecutive vectors from `first`; every vector is in exactly one pass
struct MsmBatchPass { uint32_t first, count; };
inline uint32_t msm_batch_passes(uint32_t B, uint32_t per) { return per ? (B + per - 1) / per : 0; }
inline MsmBatchPass msm_batch_pass(uint32_t B, uint32_t per, uint32_t p) {
  const uint64_t first = (uint64_t)p * per;
  if (first >= B) return {B, 0};
  return {(uint32_t)first, (uint32_t)std::min<uint64_t>(per, B - first)};
}

}  // namespace zk
