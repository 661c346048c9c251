#pragma once
// Prefix scans of Fr vectors: the geometry and the per-lane routines that the kernels of fr_scan.hip, the host hook (mi355zk_selftest_fr_scan)
// and the stand-alone host test (tests/cpp/test_fr_scan_host.cpp) share -- same source, compiled for both sides.
//
//   running products  c_1 = a_1, c_i = a_i c_{i-1}   (bellman/src/sonic/unhelped/grand_product_argument.rs:119-163, "serially for now" there)
//   running sums      s_i = a_i + s_{i-1}
// The operation is a template parameter (ScanProduct: Fr product, identity Montgomery one; ScanSum: Fr sum, identity zero), so the sum
// instantiation holds no Montgomery product at all.  A lane owns SCAN_RUN consecutive elements in registers, a workgroup of SCAN_WG lanes a
// tile, and the carry kernel walks the tile aggregates SCAN_CARRY_W at a time with a running carry, which handles any number of tiles with no
// further level.  An optional second operand is multiplied in at load: with num the element a lane scans is num[i] x[i], formed in registers.
// A zero is an ordinary element here (everything after it in a product row is zero, as in the serial chain): NOT the convention of
// fr_inverse.hpp, where a zero is skipped.
#include "fr_poly.hpp"   // poly_ld / poly_st

#include <cstring>
#include <vector>

namespace zk {

#ifndef MI355ZK_SCAN_LOG_RUN
#define MI355ZK_SCAN_LOG_RUN 4   // 16 elements: 170 VGPRs in the product's apply kernel, two waves a SIMD, and still ~20 % ahead of 8 at 2^24 (DESIGN 4d;
                                 // the other run length is a second build of fr_scan.hip, tools/bench_fr_scan.py's A/B)
#endif
constexpr int SCAN_LOG_RUN = MI355ZK_SCAN_LOG_RUN, SCAN_LOG_WG = 8, SCAN_LOG_CARRY = 8;
constexpr int SCAN_RUN = 1 << SCAN_LOG_RUN;                  // elements per lane
constexpr int SCAN_WG = 1 << SCAN_LOG_WG;                    // lanes per workgroup
constexpr int SCAN_TILE = 1 << (SCAN_LOG_RUN + SCAN_LOG_WG); // elements per workgroup
constexpr int SCAN_CARRY_W = 1 << SCAN_LOG_CARRY;            // tile aggregates per chunk of the carry kernel (its workgroup width)
static_assert(SCAN_RUN >= 2 && SCAN_RUN <= 16, "a run is held in registers: 8 VGPRs per element");

struct ScanProduct {
  ZK_HD static Fr identity() { return Fr::one(); }
  ZK_HD static Fr op(const Fr& a, const Fr& b) { return mul(a, b); }
};
struct ScanSum {
  ZK_HD static Fr identity() { return Fr::zero(); }
  ZK_HD static Fr op(const Fr& a, const Fr& b) { return add(a, b); }
};

// the run [lo, lo + SCAN_RUN) of x (times num, element by element, when num is not NULL), the identity at and past n: all the loads of the
// run are issued before the first product
template <class Op>
ZK_HD void scan_run_load(Fr v[SCAN_RUN], const Fr* x, const Fr* num, uint64_t lo, uint64_t n) {
  if (lo + SCAN_RUN <= n) {
#pragma unroll
    for (int k = 0; k < SCAN_RUN; ++k) v[k] = poly_ld(x + lo + k);
    if (num != nullptr) {
      Fr m[SCAN_RUN];
#pragma unroll
      for (int k = 0; k < SCAN_RUN; ++k) m[k] = poly_ld(num + lo + k);
#pragma unroll
      for (int k = 0; k < SCAN_RUN; ++k) v[k] = mul(m[k], v[k]);
    }
  } else {
#pragma unroll
    for (int k = 0; k < SCAN_RUN; ++k) {
      v[k] = Op::identity();
      if (lo + k < n) v[k] = num != nullptr ? mul(poly_ld(num + lo + k), poly_ld(x + lo + k)) : poly_ld(x + lo + k);
    }
  }
}
// v[0] o v[1] o .. o v[SCAN_RUN - 1]
template <class Op>
ZK_HD Fr scan_run_aggregate(const Fr v[SCAN_RUN]) {
  Fr p = v[0];
#pragma unroll
  for (int k = 1; k < SCAN_RUN; ++k) p = Op::op(p, v[k]);
  return p;
}
// the chain through the run from `seed`, the aggregate of everything before it: inclusive out[lo + k] = seed o v[0] o .. o v[k], exclusive the
// value before v[k] joins
template <class Op>
ZK_HD void scan_run_apply(Fr* out, const Fr v[SCAN_RUN], uint64_t lo, uint64_t n, Fr seed, bool exclusive) {
#pragma unroll
  for (int k = 0; k < SCAN_RUN; ++k) {
    const Fr next = Op::op(seed, v[k]);
    if (lo + k < n) poly_st(out + lo + k, exclusive ? seed : next);
    seed = next;
  }
}
// one combine step of a scan: `before` covers the positions just below those of `mine`
template <class Op>
ZK_HD Fr scan_combine(const Fr& before, const Fr& mine) { return Op::op(before, mine); }

// ---- host side: the three launches on one thread, the same runs, tiles and chunks, every combine in the kernels' order
// the log-step inclusive scan over the 2^log_w lanes of a workgroup
template <class Op>
inline void scan_lanes_host(Fr* s, int log_w) {
  const int w = 1 << log_w;
  std::vector<Fr> old(w);
  for (int k = 0; k < log_w; ++k) {
    const int d = 1 << k;
    std::memcpy(old.data(), s, sizeof(Fr) * w);
    for (int l = d; l < w; ++l) s[l] = scan_combine<Op>(old[l - d], old[l]);
  }
}
// launch 2: agg[t] (tile aggregates) -> carry[t], the aggregate of everything before tile t; returns the row's total
template <class Op>
inline Fr scan_carry_host(Fr* agg, size_t n_tiles) {
  std::vector<Fr> s(SCAN_CARRY_W);
  Fr carry = Op::identity();
  for (size_t c = 0; c * SCAN_CARRY_W < n_tiles; ++c) {
    for (int l = 0; l < SCAN_CARRY_W; ++l) {
      const size_t t = c * SCAN_CARRY_W + l;
      s[l] = t < n_tiles ? agg[t] : Op::identity();
    }
    s[0] = scan_combine<Op>(carry, s[0]);
    scan_lanes_host<Op>(s.data(), SCAN_LOG_CARRY);
    for (int l = 0; l < SCAN_CARRY_W; ++l)
      if (c * SCAN_CARRY_W + l < n_tiles) agg[c * SCAN_CARRY_W + l] = l ? s[l - 1] : carry;
    carry = s[SCAN_CARRY_W - 1];
  }
  return carry;
}
// One row on the host.  out may be in; num may be NULL.  Returns the aggregate of all n elements (the identity for n == 0).
template <class Op>
inline Fr scan_host(Fr* out, const Fr* in, const Fr* num, size_t n, bool exclusive) {
  const size_t n_tiles = (n + SCAN_TILE - 1) / SCAN_TILE;
  if (n_tiles == 0) return Op::identity();
  std::vector<Fr> carry(n_tiles, Op::identity()), s(SCAN_WG), vs((size_t)SCAN_WG * SCAN_RUN);
  Fr total = Op::identity();
  if (n_tiles > 1) {   // (a row of one tile goes through launch 3 alone)
    Fr v[SCAN_RUN];
    for (size_t t = 0; t < n_tiles; ++t) {   // launch 1
      for (int l = 0; l < SCAN_WG; ++l) {
        scan_run_load<Op>(v, in, num, (t * SCAN_WG + l) * SCAN_RUN, n);
        s[l] = scan_run_aggregate<Op>(v);
      }
      scan_lanes_host<Op>(s.data(), SCAN_LOG_WG);
      carry[t] = s[SCAN_WG - 1];
    }
    total = scan_carry_host<Op>(carry.data(), n_tiles);   // launch 2
  }
  for (size_t t = 0; t < n_tiles; ++t) {     // launch 3
    for (int l = 0; l < SCAN_WG; ++l) {      // every lane loads before any lane stores: out may be in
      Fr* v = &vs[(size_t)l * SCAN_RUN];
      scan_run_load<Op>(v, in, num, (t * SCAN_WG + l) * SCAN_RUN, n);
      s[l] = scan_run_aggregate<Op>(v);
    }
    s[0] = scan_combine<Op>(carry[t], s[0]);
    scan_lanes_host<Op>(s.data(), SCAN_LOG_WG);
    if (n_tiles == 1) total = s[SCAN_WG - 1];
    for (int l = 0; l < SCAN_WG; ++l)
      scan_run_apply<Op>(out, &vs[(size_t)l * SCAN_RUN], (t * SCAN_WG + l) * SCAN_RUN, n, l ? s[l - 1] : carry[t], exclusive);
  }
  return total;
}

#if defined(__HIPCC__)
// fr_scan.hip, for the other units of the library: `rows` rows of n elements, row r at + r * stride, scanned on `st`.  d_num (may be NULL) is
// multiplied in at load; d_total (may be NULL) receives every row's aggregate.  flags: MI355ZK_SCAN_*.  The arguments have been checked.
int fr_scan_rows(Fr* d_out, size_t out_stride, const Fr* d_in, size_t in_stride, const Fr* d_num, size_t num_stride, size_t n, size_t rows,
                 uint32_t flags, Fr* d_total, hipStream_t st);
#endif

}  // namespace zk
