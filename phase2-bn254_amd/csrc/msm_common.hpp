#pragma once
// What the Pippenger kernels (msm_partition.hip, msm_impl.hpp) and the host-side planner (msm_plan.hpp) share: the geometry structs
// that travel as kernel arguments and the compile-time limits both sides size things by.  No HIP header: the planner and the join
// compile and run without a device (tests/cpp/test_msm_host.cpp).  The structs are ordinary zk:: types, not per-unit copies: they
// cross the boundary between msm_partition.hip and the two units that include msm_host.hpp.
#include <stdint.h>

namespace zk {

constexpr uint32_t SIGN_BIT = 0x80000000u;

// Window layout.  The 254 scalar bits are split into W windows of (nearly) EQUAL width instead of W-1 full
// c-bit windows and a short remainder: a short top window would put its n digits into very few buckets
// (2^26 points, c = 20: 16383 buckets of 4096 entries against 128 everywhere else).  Windows 0..W-2 use signed
// digits (d in [-2^(width-1), 2^(width-1)], width <= c); the TOP window is at most c-1 bits wide and keeps its
// digits unsigned (value + carry <= 2^(c-1) = nb), which is also what absorbs the final carry.
struct MsmGeom {
  uint32_t c;        // bits of the sort field: bucket slots 0..nb-1, nb itself = "no bucket"
  uint32_t W;        // windows
  uint32_t nb;       // bucket slots per window (power-of-two layout: 2^(c-1); narrower windows leave their upper slots empty)
  uint8_t width[64]; // power-of-two layout: bits of window w (c >= 4: at most 64 windows)
  uint8_t shift[64]; // power-of-two layout: first bit of window w
  // MIXED-RADIX layout (rmul != 1): digits in base B = rmul * 2^rshift instead of a power of two, so that the window
  // count is not tied to whole bits -- 254 bits in 12 windows need 21.2 bits each: B = 5 * 2^19 takes 12 windows of
  // 1.31 M buckets where c = 20 takes 13 (one accumulation pass and one sort-pass share less) and c = 22 would pay
  // 2.1 M buckets per window in the reduction.  k = sum_w d_w B^w, d_w in (-B/2, B/2], top digit unsigned <= nb = B/2.
  uint32_t rmul;     // 1 (power-of-two layout) or an odd multiplier 3..15
  uint32_t rshift;
};

// partition (msm_partition.hip, section 2)
constexpr uint32_t MSM_SIZE_BINS = 4096;   // bins of the counting sort that orders the buckets by size (3b)
constexpr uint32_t PART_THREADS = 1024;
constexpr uint32_t PART_MAX_ST = 16384;       // super-tile: scalars per pass-A histogram dump = elements per pass-B workgroup
constexpr uint32_t PART_MAX_EB = PART_MAX_ST / PART_THREADS;
constexpr uint32_t PART_LO_MAX = 12;          // at most 4096 buckets per coarse bin
constexpr uint32_t PART_EC = 32;              // pass C: elements per lane held in registers
constexpr uint32_t PART_LDS_A = 76 * 1024;    // pass A histogram budget (16-bit counters; two workgroups per CU)
constexpr uint32_t PART_LDS_MAX = 160 * 1024 - 512;
constexpr uint32_t KEY_NONE_MASK = 0x00ffffffu;  // key = bucket (or nb = none) in the low 24 bits | SIGN_BIT

struct PartGeom {
  uint32_t lo_bits;   // fine bits: buckets per coarse bin = 2^lo_bits
  uint32_t nbin;      // coarse bins per window
  uint32_t st;        // super-tile size (multiple of PART_THREADS)
  uint32_t n_st;      // super-tiles
  uint32_t n_chunk;   // row chunks of the column scans
  uint32_t rows_per_chunk;
};

constexpr uint32_t BIG_SEG = PART_EC * PART_THREADS;   // elements per segment of a big bin (msm_bigbin_*)

struct BigPlan {         // device-side
  uint32_t n_big;        // big bins
  uint32_t total_seg;    // their segments
};

// accumulation (sections 4, 4a)
constexpr uint32_t MSM_HEAVY_BLOCKS = 65536;  // at most this many buckets take the segment-parallel path (the rest of a pathological input runs one lane per bucket)
constexpr uint32_t MSM_HEAVY_SEG = 4096;    // entries per segment at size; short calls cut finer (heavy_seg_for)
constexpr uint32_t MSM_HEAVY_LANES = 64;   // one wave per segment: 64 strided partial sums of <= 64 points, then a 6-level tree
constexpr uint32_t MSM_PAIR_MAX_BUCKETS = 3u << 17;   // (2^18 points: 17 windows x 2^14 buckets = 278 k -> pairs; 2^19: 16 x 2^15 = 524 k -> lanes)

// reduction (section 5)
constexpr uint32_t MSM_FINAL_MAX = 1024;  // (2048 and 8192 measured in round 2: the bit-decomposition trees cost more than the level they replace)
constexpr uint32_t MSM_TREE_SLICE = 512;
constexpr uint32_t MSM_MAX_LEVELS = 8;
constexpr uint32_t MSM_MAX_JOBS = MSM_MAX_LEVELS + 24;

// a BATCH: n_vectors exponent vectors of n exponents over ONE base vector and ONE density map (msm_plan.hpp: MsmRequest::n_vectors, msm_batch_split)
// What bounds the bucket sets WL = B * WD of one pipeline pass, from the uses of WL, ncell and n_buckets in the planner, the partition,
// the accumulation and the reduction (none of them indexes MsmGeom::width / shift by a bucket set: those are per window of ONE vector):
//   u32 products      n_buckets = WL * nb, m = n * WL and the index lists' vals_cap <= 0xfffffff0; the grids n_st * WL, lvl_chunks * WL and
//                     first_block[n_jobs] * WL (the last one checked as such; the others are below m and n_buckets)
//   choose_part       fits_lds: WL * nbin 16-bit counters within 2 * PART_LDS_A at the coarsest bins (nbin = ceil(nb / 4096)): 77824 / nbin sets
//   gates, not limits small_scan (n_st * ncell <= 2^16), quad_max_chunks, MSM_PAIR_MAX_BUCKETS and the split launch only choose between kernels
//                     that all take any WL; MSM_HEAVY_BLOCKS caps the buckets of the segment-parallel path, the others run a lane each
//   back_bytes()      WL * n_out records come back through ONE pinned buffer, grow-only and one per concurrent caller (the prover has eight):
//                     4096 sets x 30 records x 256 B (G2) = 30 MiB.  THIS is the binding one for short vectors -- at n <= 2^13 the u32 and
//                     LDS limits allow 2^16 sets and more -- and it sets the constant; from ~2^18 exponents on the workspace itself binds first
//                     (MSM_BATCH_WS_MAX: a 2^20-point G1 batch of 16 vectors is 256 sets and 5 GiB of keys, pairs and bucket records).
constexpr uint32_t MSM_BATCH_MAX_WINDOWS = 4096;       // bucket sets per pipeline pass
constexpr uint64_t MSM_BATCH_WS_MAX = (uint64_t)8 << 30;  // workspace bytes per pipeline pass

}  // namespace zk
