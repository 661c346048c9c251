#pragma once
// Division of an Fr polynomial by (x - z) and its evaluation at z: the geometry and the per-lane routines that the kernels of fr_poly.hip
// and the host hook (mi355zk_selftest_fr_poly_divide) share -- same source, compiled for both.
//
//   kate_divison (bellman/src/sonic/util.rs:444-463):  q[n-2] = a[n-1],  q[i-1] = a[i] + z q[i];  the step below q[0] is the remainder a(z).
// With H[i] = sum_{k >= 0} a[i+k] z^k (a[j] = 0 for j >= n) that is q[i-1] = H[i] and a(z) = H[0]: a suffix scan of the affine recurrence
// H[i] = a[i] + z H[i+1], whose multiplier over a distance d is z^d whatever the position.  Every lane owns POLY_RUN consecutive
// coefficients, a workgroup POLY_TILE, and the carry kernel walks the tiles POLY_CARRY_W at a time; all three are powers of two, so every
// multiplier that a combine step needs is one of the squarings sq[j] = z^(2^j) and no general power of z is ever formed.
#include "field.hpp"

namespace zk {

#ifndef MI355ZK_POLY_LOG_RUN
#define MI355ZK_POLY_LOG_RUN 4   // (a build-time constant: tools/bench_kzg.py's A/B of another run length is a second build of this unit)
#endif
constexpr int POLY_LOG_RUN = MI355ZK_POLY_LOG_RUN, POLY_LOG_WG = 8, POLY_LOG_CARRY = 8;
constexpr int POLY_RUN = 1 << POLY_LOG_RUN;          // coefficients per lane
constexpr int POLY_WG = 1 << POLY_LOG_WG;            // lanes per workgroup
constexpr int POLY_LOG_TILE = POLY_LOG_RUN + POLY_LOG_WG;
constexpr int POLY_TILE = 1 << POLY_LOG_TILE;        // coefficients per workgroup
constexpr int POLY_CARRY_W = 1 << POLY_LOG_CARRY;    // tiles per chunk of the carry kernel (its workgroup width)
constexpr int POLY_SQ = POLY_LOG_TILE + POLY_LOG_CARRY;
static_assert(POLY_RUN <= 16, "a run is held in registers: 8 VGPRs per coefficient");

// sq[j] = z^(2^j): the lane scan of a tile uses sq[POLY_LOG_RUN + k] at distance 2^k lanes, the tile scan sq[POLY_LOG_TILE + k] at 2^k tiles
struct FrPolyPoint {
  Fr sq[POLY_SQ];
};
ZK_HD void poly_point_fill(FrPolyPoint& t, const Fr& z) {
  t.sq[0] = z;
  for (int j = 1; j < POLY_SQ; ++j) t.sq[j] = sqr(t.sq[j - 1]);
}

ZK_HD Fr poly_ld(const Fr* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* q = reinterpret_cast<const uint4*>(p);
  const uint4 a = q[0], b = q[1];
  Fr r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  return r;
#else
  return *p;
#endif
}
ZK_HD void poly_st(Fr* p, const Fr& v) {
#if defined(__HIP_DEVICE_COMPILE__)
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
#else
  *p = v;
#endif
}

// the run [lo, lo + POLY_RUN) of a, zero at and past n: all the loads are issued before the first product
ZK_HD void poly_run_load(Fr v[POLY_RUN], const Fr* a, uint64_t lo, uint64_t n) {
  if (lo + POLY_RUN <= n) {
#pragma unroll
    for (int k = 0; k < POLY_RUN; ++k) v[k] = poly_ld(a + lo + k);
  } else {
#pragma unroll
    for (int k = 0; k < POLY_RUN; ++k) v[k] = lo + k < n ? poly_ld(a + lo + k) : Fr::zero();
  }
}
// H at the bottom of the run, given H just above it (`seed`): one product and one addition per coefficient
ZK_HD Fr poly_run_value(const Fr v[POLY_RUN], const Fr& z, Fr seed) {
#pragma unroll
  for (int k = POLY_RUN - 1; k >= 0; --k) seed = add(mul(seed, z), v[k]);
  return seed;
}
// the same chain with every step stored: H[lo + k] is q[lo + k - 1], for 1 <= lo + k <= n - 1
ZK_HD void poly_run_apply(Fr* q, const Fr v[POLY_RUN], uint64_t lo, uint64_t n, const Fr& z, Fr seed) {
#pragma unroll
  for (int k = POLY_RUN - 1; k >= 0; --k) {
    seed = add(mul(seed, z), v[k]);
    const uint64_t i = lo + k;
    if (i >= 1 && i < n) poly_st(q + i - 1, seed);
  }
}
// one combine step of a suffix scan: `mine` covers 2^k positions, `up` the 2^k above them, m = the multiplier across 2^k positions
ZK_HD Fr poly_combine(const Fr& mine, const Fr& m, const Fr& up) { return add(mine, mul(m, up)); }

}  // namespace zk
