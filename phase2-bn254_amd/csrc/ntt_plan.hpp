#pragma once
// The host-side PLAN of a transform (ntt.hip: ntt_run_batch): the factoring of the index into passes, which table arrangement feeds
// each of the pass kernel's table arguments, and every launch's geometry -- pure arithmetic on the request and the knobs.  No HIP call
// and no getenv below ntt_knobs(): the planner runs, and is tested, without a device (tests/test_ntt_plan_host.py).
// Also here, because both the kernels and the planner need them: NttPassParams, NttBatch and the NTT_* constants.
#include <stdint.h>

#include <cstddef>
#include <cstdlib>

#include "field.hpp"
#include "host_util.hpp"

namespace zk {

namespace {

constexpr int NTT_MAX_LOG_NP = 12;   // longest sub-transform a tile row can be (kernel instantiations, root tables)
constexpr int NTT_LOG_NP = 10;       // the pass planner's default: 1024-point rows (longer ones for 2^21 .. 2^23; env MI355ZK_NTT_LOGNP = 10 / 11 / 12 forces)
constexpr int NTT_TILE_ELEMS = 4096; // G * N_p
constexpr int NTT_THREADS = 1024;
constexpr size_t NTT_LDS_BYTES_MAX = 160 * 1024;  // gfx950: 160 KiB of LDS per CU; the tile kernels stage up to 4096 x 36 B = 144 KiB of it
constexpr uint32_t NTT_FULL_TW_MAX_LOG = 20;      // the largest two-pass transform that streams a full inter-pass table (ntt_plan: full_tw)

struct NttPassParams {
  uint32_t log_np;       // log2(N_p)
  uint32_t g;            // rows (batch) per tile
  uint64_t in_xs, in_gs; // element strides (in elements) of transform index / batch index on load
  uint64_t out_xs, out_gs;
  // tile -> base offsets: tile id = hi * tiles_lo + lo
  uint64_t tiles_lo;
  uint64_t in_hi_stride, in_lo_stride;
  uint64_t out_hi_stride, out_lo_stride;
  uint32_t load_x_fastest;  // lane order on load: 1 = transform index fastest (last pass)
  // inter-pass twiddle  w^(tw_mul * k * (lo*g + gidx)) ; tw_mul == 0 -> none (last pass)
  uint64_t tw_mul;
  uint32_t tw_h;            // two-level split: w^e = A[e >> h] * B[e & (2^h - 1)]
  uint32_t tw_full;         // 1: the first pass of a two-pass transform reads its twiddle w^(k * col) from a table indexed by the OUTPUT position
  uint32_t pre;             // first pass of coset_fft: element i *= g^i   (1: preA/preB, split pre_h; round 5, folded tables: 2: row position x *= preA[x];
                            // 3: butterfly twiddles from the stage table preA (wave-local kernel); 4: that, and *= preB[col])
  uint32_t pre_h;
  uint32_t post;            // last pass: 1 = multiply by post_c; 2 = by post_c * ginv^k (postA/postB, split post_h); 3 = by nothing; 4 = row output k *= postA[k]; 5 = that, and *= postB[first output index of the row]
  uint32_t post_h;
  uint32_t xcd_pair;        // 1: tiles 2j and 2j + 1 run on the same XCD, one dispatch round apart (see the kernel)
  // (round 5) batch > 1: ONE launch runs this pass of `batch` independent transforms of the same size and kind: workgroup ids
  // [t * tiles, (t + 1) * tiles) belong to transform t, whose arrays are NttBatch::in[t] / out[t]
  uint32_t batch;
  uint64_t tiles;
};
constexpr uint32_t NTT_MAX_BATCH = 8;
struct NttBatch {
  const Fr* in[NTT_MAX_BATCH];
  Fr* out[NTT_MAX_BATCH];
};

// Every environment knob of the NTT's host side, read in ONE place (ntt_knobs), once per process; the planner and the table cache take
// them as an argument.  Experiment / comparison switches unless noted; the defaults below are what an empty environment gives.
struct NttKnobs {
  int lognp = 0;               // MI355ZK_NTT_LOGNP = 10 / 11 / 12: rows of that length for every size (0: the planner's own choice)
  int tile = 0;                // MI355ZK_NTT_TILE = 4096 / 2048 / 1024: elements per tile (0: by size)
  int radix = 0;               // MI355ZK_NTT_RADIX = 4: radix-4 register butterflies for every tile; any other value: radix-2 (0: by tile size)
  bool no_wavelocal = false;   // MI355ZK_NTT_WAVELOCAL = 0: the barrier-per-pair kernel where the wave-local one would run, for the A/B
  bool no_full_tw = false;     // MI355ZK_NTT_NO_FULL_TW: the two-level product instead of the full inter-pass table, kept for the comparison in DESIGN.md
  bool no_fold = false;        // MI355ZK_NTT_NO_FOLD: the separate scale products of rounds 1-4 instead of folded tables, for the A/B
  bool no_stage_fold = false;  // MI355ZK_NTT_NO_STAGE_FOLD: a folded coset transform keeps its row twist as a product at the load (pre == 2), not in the butterflies
  bool no_pair = false;        // MI355ZK_NTT_NOPAIR: no XCD grouping of neighbouring tiles
  uint32_t pair = 5;           // MI355ZK_NTT_PAIR = 1 / 5: which grouping (NttPassParams::xcd_pair)
  bool pair_all = false;       // MI355ZK_NTT_PAIR_ALL: group the tiles of wide-tile passes too
  double tables_gb = 4.0;      // MI355ZK_NTT_TABLES_GB: per-device byte budget of the table cache (ntt_tables.hpp), at least 32 MiB.  A setting, not an experiment
};

inline const NttKnobs& ntt_knobs() {
  static const NttKnobs process = [] {
    NttKnobs K;
    auto num = [](const char* name) { const char* s = std::getenv(name); return s ? std::atoi(s) : 0; };
    auto set = [](const char* name) { return std::getenv(name) != nullptr; };
    if (num("MI355ZK_NTT_LOGNP") >= 10 && num("MI355ZK_NTT_LOGNP") <= 12) K.lognp = num("MI355ZK_NTT_LOGNP");
    const int tile = num("MI355ZK_NTT_TILE");
    if (tile == 2048 || tile == 4096 || tile == 1024) K.tile = tile;
    if (set("MI355ZK_NTT_RADIX")) K.radix = num("MI355ZK_NTT_RADIX") == 4 ? 4 : 2;
    if (const char* s = std::getenv("MI355ZK_NTT_WAVELOCAL")) K.no_wavelocal = s[0] == '0';
    K.no_full_tw = set("MI355ZK_NTT_NO_FULL_TW");
    K.no_fold = set("MI355ZK_NTT_NO_FOLD");
    K.no_stage_fold = set("MI355ZK_NTT_NO_STAGE_FOLD");
    K.no_pair = set("MI355ZK_NTT_NOPAIR");
    if (set("MI355ZK_NTT_PAIR")) K.pair = (uint32_t)num("MI355ZK_NTT_PAIR");
    K.pair_all = set("MI355ZK_NTT_PAIR_ALL");
    if (const char* s = std::getenv("MI355ZK_NTT_TABLES_GB")) K.tables_gb = std::atof(s);
    return K;
  }();
  return process;
}

// a[i] *= pre_g^i (if pre_g)  ->  X = NTT(a)  ->  X[k] *= post_c * post_g^k (if given), for `batch` arrays of 2^log_n elements
struct NttRequest {
  uint32_t log_n = 0;
  uint32_t batch = 1;
  bool pre_g = false, post_c = false, post_g = false;
};

// which kernel runs a pass (ntt.hip: the table of kernels is indexed by this and the row length)
enum NttKernelKind : uint32_t { NTT_KERNEL_R2 = 0, NTT_KERNEL_R4 = 1, NTT_KERNEL_WL = 2, NTT_KERNEL_KINDS = 3 };  // radix-2 barrier, radix-4 barrier, wave-local

enum NttBuf : uint32_t { NTT_BUF_ARRAY = 0, NTT_BUF_SCRATCH = 1 };  // the caller's array(s) / the per-stream scratch

// Where a table argument of a pass kernel comes from.  T, Tpre, Tpost: the two-level power tables (PowTables) of omega, pre_g and post_g;
// F: the folded set of (omega, pre_g, post_c, post_g) (PowTables::Folded).
enum NttTab : uint32_t {
  NTT_TAB_NULL = 0,
  NTT_TAB_T_A, NTT_TAB_T_B, NTT_TAB_T_FULL,
  NTT_TAB_TPRE_A, NTT_TAB_TPRE_B, NTT_TAB_TPOST_A, NTT_TAB_TPOST_B,
  NTT_TAB_F_FULL, NTT_TAB_F_PRE_ROWS, NTT_TAB_F_PRE_STAGES, NTT_TAB_F_PRE_COLS, NTT_TAB_F_POST_ROWS, NTT_TAB_F_POST_ROWC, NTT_TAB_F_TW_B_SCALED,
  NTT_TAB_COUNT
};
inline const char* ntt_tab_name(NttTab t) {
  static const char* const names[NTT_TAB_COUNT] = {"null", "T.A", "T.B", "T.full", "Tpre.A", "Tpre.B", "Tpost.A", "Tpost.B", "F.full", "F.pre_rows",
                                                   "F.pre_stages", "F.pre_cols", "F.post_rows", "F.post_rowc", "F.tw_b_scaled"};
  return t < NTT_TAB_COUNT ? names[t] : "?";
}
inline bool ntt_tab_is_folded(NttTab t) { return t >= NTT_TAB_F_FULL && t < NTT_TAB_COUNT; }

// the pass kernels' table arguments, in the kernels' order (`roots` is always T.roots[log_np] and is not listed)
enum NttArg : uint32_t { NTT_ARG_TW_A = 0, NTT_ARG_TW_B, NTT_ARG_PRE_A, NTT_ARG_PRE_B, NTT_ARG_POST_A, NTT_ARG_POST_B, NTT_ARG_TW_F, NTT_ARGS };

struct NttPass {
  NttPassParams P;        // (P.log_np is the kernel's LOG_NP)
  NttKernelKind kind;
  uint32_t threads;
  uint32_t grid;          // P.tiles * P.batch
  size_t lds_bytes;
  NttBuf src, dst;
  NttTab tab[NTT_ARGS];
};

struct NttPlan {
  int R;                  // passes
  uint32_t b[3];          // bits of the index pass p transforms, b[0] the most significant digit
  uint32_t h;             // every two-level table of this size splits its exponent at h bits (PowTables::h)
  bool full_tw;           // a two-pass transform whose first pass streams its inter-pass twiddles from a full table
  bool fold;              // ... and that table has the transform's scale factors folded in (F.full)
  bool fold_big;          // no full table (2^21 and up), the small folded tables of the same split
  // what the launcher has to find or build before it resolves the passes' tables: T with roots[b[0 .. R)] always, and
  uint32_t full_log_s;    // T.full for this split's column count (0: not wanted)
  bool want_tpre, want_tpost;  // Tpre / Tpost
  bool want_folded;       // F, with its full table (fold) or without (fold_big); its members, as build_folded makes them:
  uint32_t folded_members;  // bit (1 << NttTab) for every F.* table the set holds
  bool want_scratch;      // batch * 2^log_n elements of inter-pass scratch
  NttPass pass[3];
};

// Refusals (ZK_ERR_BAD_ARGS): batch 0 or above NTT_MAX_BATCH, log_n > 30, a row length with no kernel.  log_n == 0 is no refusal: it is
// the launcher's early exit (a single element has no pass) and plans R = 0 passes here.
inline int ntt_plan(const NttRequest& Q, const NttKnobs& K, NttPlan* out) {
  if (Q.batch == 0 || Q.batch > NTT_MAX_BATCH) return ZK_ERR_BAD_ARGS;
  if (Q.log_n > 30) return ZK_ERR_BAD_ARGS;
  NttPlan& N = *out;
  N = NttPlan{};
  const uint32_t log_n = Q.log_n;
  const uint64_t n = 1ull << log_n;
  // factor the index: R passes of b[p] bits, b[0] most significant digit (DESIGN.md "NTT")
  // rows of 2^10 by default; 2^11 / 2^12 where that saves a whole pass: 2^21 and 2^22 in two passes (0.372 -> 0.294 ms, 0.715 ->
  // 0.57 ms), 2^23 as 12 + 11 (1.36 -> 1.18 ms).  The one- and two-row tiles of those passes move 32- / 64-byte runs; the kernel's
  // XCD grouping of neighbouring tiles is what makes them pay.  2^24 ran as 12 + 12 in round 2 (2.43 ms); with two 2048-element
  // workgroups per CU three passes of 2^8-point rows are faster (2.32 ms) than two passes whose 4096-point rows own a CU each.
  uint32_t row_bits = NTT_LOG_NP;
  if (log_n == 21 || log_n == 22) row_bits = 11;
  if (log_n == 23) row_bits = 12;
  if (K.lognp) row_bits = (uint32_t)K.lognp;
  const int R = (int)((log_n + row_bits - 1) / row_bits);
  uint32_t* const b = N.b;
  for (int p = 0; p < R; ++p) b[p] = log_n / R + ((uint32_t)p < log_n % R ? 1 : 0);
  N.R = R;
  N.h = (log_n + 1) / 2;

  // Measured (round 3): 2^20 fft 0.1507 -> 0.1456 ms with the full table (one product less per element of the first pass, 50 MB more to
  // stream); at 2^22 the 192 MiB table makes the transform SLOWER (0.564 -> 0.580 ms): the pass is VALU-bound only while its streams stay
  // inside the L2 / Infinity Cache.  Hence two-pass transforms up to 2^20 (NTT_FULL_TW_MAX_LOG) only.
  const bool scaled = Q.pre_g || Q.post_c || Q.post_g;
  const bool full_tw = R == 2 && log_n <= NTT_FULL_TW_MAX_LOG && !K.no_full_tw;
  // (round 5) a scaled two-pass transform with a full table takes that table with its scale factors folded in (ntt_full_folded_kernel)
  const bool fold = full_tw && !K.no_fold && scaled;
  // ... and from 2^21 on (no full table; every pass a full tile of the wave-local kernel) the small tables of the same split
  const bool fold_big = !full_tw && R >= 2 && log_n >= 21 && !K.no_fold && scaled;
  // a transform scaled by post_c alone: the pass before the last multiplies it in with its twiddle (the low table B times post_c), the
  // last pass by nothing.  Decided for both passes together, whichever kernel runs them: post == 3 is in both.
  const bool post_c_rides = fold_big && Q.post_c && !Q.post_g;
  N.full_tw = full_tw;
  N.fold = fold;
  N.fold_big = fold_big;
  N.full_log_s = (full_tw && !fold) ? b[1] : 0;
  N.want_tpre = Q.pre_g;
  N.want_tpost = Q.post_g;
  N.want_folded = fold || fold_big;
  N.want_scratch = R > 1;
  if (N.want_folded) {  // (ntt_tables.hpp: build_folded)
    auto bit = [](NttTab t) { return 1u << t; };
    if (Q.pre_g) N.folded_members |= bit(NTT_TAB_F_PRE_ROWS) | bit(NTT_TAB_F_PRE_STAGES) | (fold ? 0u : bit(NTT_TAB_F_PRE_COLS));
    if (Q.post_g) N.folded_members |= bit(NTT_TAB_F_POST_ROWS) | (fold ? 0u : bit(NTT_TAB_F_POST_ROWC));
    else if (Q.post_c && !fold) N.folded_members |= bit(NTT_TAB_F_TW_B_SCALED);
    if (fold) N.folded_members |= bit(NTT_TAB_F_FULL);
  }

  // the table arguments every pass gets unless its kernel and position say otherwise (below): the two-level tables, or with a folded full
  // table the row tables that go with it
  NttTab base[NTT_ARGS];
  base[NTT_ARG_TW_A] = NTT_TAB_T_A;
  base[NTT_ARG_TW_B] = NTT_TAB_T_B;
  base[NTT_ARG_PRE_A] = !Q.pre_g ? NTT_TAB_NULL : fold ? NTT_TAB_F_PRE_ROWS : NTT_TAB_TPRE_A;
  base[NTT_ARG_PRE_B] = (Q.pre_g && !fold) ? NTT_TAB_TPRE_B : NTT_TAB_NULL;
  base[NTT_ARG_POST_A] = !Q.post_g ? NTT_TAB_NULL : fold ? NTT_TAB_F_POST_ROWS : NTT_TAB_TPOST_A;
  base[NTT_ARG_POST_B] = (Q.post_g && !fold) ? NTT_TAB_TPOST_B : NTT_TAB_NULL;
  base[NTT_ARG_TW_F] = fold ? NTT_TAB_F_FULL : full_tw ? NTT_TAB_T_FULL : NTT_TAB_NULL;

  // tile size: 2048 elements (72 KiB of LDS, 512 lanes with a group of four each: TWO workgroups per CU, whose barriers tie eight
  // waves instead of sixteen and whose load / compute / store phases may drift apart) for transforms of 2^20 and more; rows of 2^12
  // are a tile of their own.  Round 2 measured 2048-element tiles 2-5 % SLOWER -- but with radix-2 stages on 1024-lane workgroups,
  // of which the registers (125 VGPRs) admit one per CU: that was never two workgroups per CU.  With a lane per group of four:
  // 2^20 0.1474 -> 0.1443 ms (ifft 0.1418 -> 0.1386), 2^22 0.569 -> 0.544 (ifft 0.536 -> 0.498).
  const uint64_t tile_elems = K.tile ? (uint64_t)K.tile : log_n >= 20 ? 2048 : NTT_TILE_ELEMS;
  // S[p] = prod_{q>p} N_q ; Tm[p] = prod_{q<p} N_q
  uint64_t S[3], Tm[3];
  for (int p = 0; p < R; ++p) {
    S[p] = 1;
    Tm[p] = 1;
    for (int q = p + 1; q < R; ++q) S[p] <<= b[q];
    for (int q = 0; q < p; ++q) Tm[p] <<= b[q];
  }

  for (int p = 0; p < R; ++p) {
    NttPass& pass = N.pass[p];
    NttPassParams& P = pass.P;
    P.log_np = b[p];
    const uint64_t np = 1ull << b[p];
    const bool first = p == 0, last = p == R - 1;
    pass.src = first ? NTT_BUF_ARRAY : NTT_BUF_SCRATCH;
    pass.dst = last ? NTT_BUF_ARRAY : NTT_BUF_SCRATCH;
    uint64_t tiles;
    if (!last || R == 1) {
      // columns: G adjacent low positions share a tile
      uint64_t G = tile_elems / np;
      if (G < 1) G = 1;
      if (G > S[p]) G = S[p];
      while (G > 1 && n / (np * G) < 256) G >>= 1;  // small transforms: prefer >= 256 tiles (one per CU) over wide tiles
      P.g = (uint32_t)G;
      P.in_xs = P.out_xs = S[p];
      P.in_gs = P.out_gs = 1;
      P.tiles_lo = S[p] / G;
      P.in_hi_stride = P.out_hi_stride = np * S[p];
      P.in_lo_stride = P.out_lo_stride = G;
      P.load_x_fastest = (G == 1);
      P.tw_mul = (R == 1) ? 0 : Tm[p];
      P.tw_h = N.h;
      P.tw_full = (full_tw && first) ? 1u : 0u;  // (p == 0 of R == 2: Tm = 1, hi = 0, so the output position is k * S + col)
      tiles = Tm[p] * P.tiles_lo;
    } else {
      // last pass: G rows with adjacent k_1; hi = k_1 group, lo = middle digit (R == 3) else 0
      const uint64_t N1 = 1ull << b[0];
      uint64_t G = tile_elems / np;
      if (G < 1) G = 1;
      if (G > N1) G = N1;
      while (G > 1 && n / (np * G) < 256) G >>= 1;
      P.g = (uint32_t)G;
      P.in_xs = 1;
      P.in_gs = S[0];
      P.out_xs = n >> b[p];
      P.out_gs = 1;
      const uint64_t mid = (R == 3) ? (1ull << b[1]) : 1;
      P.tiles_lo = mid;
      P.in_hi_stride = G * S[0];
      P.in_lo_stride = np;      // middle digit k_2 sits at stride S[1] = N_3 = np
      P.out_hi_stride = G;
      P.out_lo_stride = N1;     // k_2 * T_2 = k_2 * N_1
      P.load_x_fastest = 1;
      P.tw_mul = 0;
      tiles = (N1 / G) * mid;
    }
    P.batch = Q.batch;
    P.tiles = tiles;
    pass.grid = (uint32_t)(tiles * Q.batch);
    // (narrow tiles only: with 128-byte runs and more the grouping is neutral -- measured with MI355ZK_NTT_PAIR_ALL)
    P.xcd_pair = ((P.g <= 2 || K.pair_all) && tiles % 256 == 0 && !K.no_pair) ? K.pair : 0u;

    const uint64_t elems = (uint64_t)P.g * np;
    pass.lds_bytes = (size_t)elems * 36;
    // One instantiation per row length: static stage loops.  Radix-4 register butterflies, a lane per group of four, for full tiles
    // (>= 2048 elements: transforms of 2^20 and more), radix-2 for the narrow tiles of short transforms, whose passes are latency-bound
    // and want two butterflies per lane rather than half the lanes idle.
    const bool r4 = K.radix ? K.radix == 4 : elems >= 2048;
    uint32_t threads = (uint32_t)(elems / (r4 ? 4 : 2));
    if (threads > NTT_THREADS) threads = NTT_THREADS;
    if (threads < 64) threads = 64;
    pass.threads = threads;
    // full tiles of rows of >= 256 elements: the wave-local kernel (round 5)
    const bool wl = r4 && !K.no_wavelocal && b[p] >= 8 && elems == 4ull * threads;
    pass.kind = wl ? NTT_KERNEL_WL : r4 ? NTT_KERNEL_R4 : NTT_KERNEL_R2;
    if (b[p] < (wl ? 8u : 1u) || b[p] > (uint32_t)NTT_MAX_LOG_NP) return ZK_ERR_BAD_ARGS;  // a row length with no kernel

    // the scale factors and the tables they come from.  The barrier kernels know pre 1 / 2 and post 1 .. 4 and get the base tables; the
    // stage table (pre 3 / 4) and the row constants (post 5) are the wave-local kernel's alone.
    for (uint32_t a = 0; a < NTT_ARGS; ++a) pass.tab[a] = base[a];
    if (first && Q.pre_g) {
      P.pre = fold ? 2 : 1;
      P.pre_h = N.h;
      if (fold && wl && !K.no_stage_fold) { P.pre = 3; pass.tab[NTT_ARG_PRE_A] = NTT_TAB_F_PRE_STAGES; }
      if (fold_big && wl) { P.pre = 4; pass.tab[NTT_ARG_PRE_A] = NTT_TAB_F_PRE_STAGES; pass.tab[NTT_ARG_PRE_B] = NTT_TAB_F_PRE_COLS; }
    }
    if (last) {
      if (fold) P.post = Q.post_g ? 4 : 3;    // post_c (and post_g^k1) sit in the folded table
      else P.post = Q.post_g ? 2 : (Q.post_c ? 1 : 3);
      P.post_h = Q.post_g ? N.h : 0;
      if (fold_big && wl && Q.post_g) { P.post = 5; pass.tab[NTT_ARG_POST_A] = NTT_TAB_F_POST_ROWS; pass.tab[NTT_ARG_POST_B] = NTT_TAB_F_POST_ROWC; }
      if (post_c_rides) P.post = 3;
    }
    if (post_c_rides && p == R - 2) pass.tab[NTT_ARG_TW_B] = NTT_TAB_F_TW_B_SCALED;
  }
  return ZK_OK;
}

}  // namespace

}  // namespace zk
