#pragma once
// Batch inversion of Fr by Montgomery's trick: the geometry and the per-lane routines that the kernels of fr_inverse.hip, the host hook
// (mi355zk_selftest_fr_batch_inverse) and the stand-alone host test (tests/cpp/test_fr_inverse_host.cpp) share -- same source, compiled
// for both sides.
//
// One inversion buys many: with P = x_0 x_1 .. x_{m-1} and J = P^-1, x_{m-1}^-1 = (x_0 .. x_{m-2}) J and J x_{m-1} is the inverse of the
// shorter product.  A lane owns INV_RUN consecutive elements in registers, a workgroup of INV_WG lanes a tile.  The lanes of a tile meet in
// a binary PRODUCT TREE of 2 INV_WG nodes (heap order: node i has the children 2 i and 2 i + 1, the lanes' run products are the leaves
// INV_WG + lane, node 1 is the tile's product).  Going up a node becomes the product of its children; once node 1 holds the INVERSE of the
// tile's product, going down a child becomes (its parent's inverse) (its sibling's product) -- its own inverse -- so the leaves end as the
// inverses of the run products, at one product per node each way and log2 INV_WG dependent steps.  The same tree, INV_CARRY_W wide, turns
// tile products into tile inverses (launch 2 of fr_inverse.hip).
// A zero element enters every product as one and is written back as zero: two selects, no branch.
#include "fr_poly.hpp"   // poly_ld / poly_st

#include <vector>

namespace zk {

#ifndef MI355ZK_INV_LOG_RUN
#define MI355ZK_INV_LOG_RUN 3   // 8 elements: the run and its prefix products are 2 x 64 VGPRs, which leaves three waves a SIMD
#endif
#ifndef MI355ZK_INV_ONE_LAUNCH
#define MI355ZK_INV_ONE_LAUNCH 0   // 1: variant (b), every tile inverts its own product in one launch (the A/B build of tools/bench_kzg_evals.py)
#endif
constexpr int INV_LOG_RUN = MI355ZK_INV_LOG_RUN, INV_LOG_WG = 8, INV_LOG_CARRY = 9;
constexpr int INV_RUN = 1 << INV_LOG_RUN;                 // elements per lane
constexpr int INV_WG = 1 << INV_LOG_WG;                   // lanes per workgroup
constexpr int INV_TILE = 1 << (INV_LOG_RUN + INV_LOG_WG); // elements per workgroup
constexpr int INV_CARRY_W = 1 << INV_LOG_CARRY;           // tile products per chunk of launch 2 (its workgroup width)
constexpr bool INV_ONE_LAUNCH = MI355ZK_INV_ONE_LAUNCH != 0;
static_assert(INV_RUN >= 2 && INV_RUN <= 16, "a run and its prefix products are held in registers: 16 VGPRs per element");

ZK_HD Fr inv_select(bool take_b, const Fr& a, const Fr& b) {
  Fr r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.l[i] = take_b ? b.l[i] : a.l[i];
  return r;
}

// the run [lo, lo + INV_RUN) of a: a zero element, and every position at or past n, is held as one; bit k of the result: a[lo + k] == 0
ZK_HD uint32_t inv_run_load(Fr v[INV_RUN], const Fr* a, uint64_t lo, uint64_t n) {
  const Fr one = Fr::one();
  if (lo + INV_RUN <= n) {
#pragma unroll
    for (int k = 0; k < INV_RUN; ++k) v[k] = poly_ld(a + lo + k);
  } else {
#pragma unroll
    for (int k = 0; k < INV_RUN; ++k) v[k] = lo + k < n ? poly_ld(a + lo + k) : one;
  }
  uint32_t zeros = 0;
#pragma unroll
  for (int k = 0; k < INV_RUN; ++k) {
    const bool z = v[k].is_zero();
    zeros |= (z ? 1u : 0u) << k;
    v[k] = inv_select(z, v[k], one);
  }
  return zeros;
}
// forward products: pre[k] = v[0] v[1] .. v[k]; pre[INV_RUN - 1] is the run's product
ZK_HD void inv_run_prefix(Fr pre[INV_RUN], const Fr v[INV_RUN]) {
  pre[0] = v[0];
#pragma unroll
  for (int k = 1; k < INV_RUN; ++k) pre[k] = mul(pre[k - 1], v[k]);
}
ZK_HD Fr inv_run_product(const Fr v[INV_RUN]) {
  Fr p = v[0];
#pragma unroll
  for (int k = 1; k < INV_RUN; ++k) p = mul(p, v[k]);
  return p;
}
// back-substitution from J = (the run's product)^-1: out[k] = pre[k - 1] J, J *= v[k]; zero where the input was
ZK_HD void inv_run_apply(Fr* out, const Fr v[INV_RUN], const Fr pre[INV_RUN], uint32_t zeros, uint64_t lo, uint64_t n, Fr J) {
  const Fr zero = Fr::zero();
#pragma unroll
  for (int k = INV_RUN - 1; k >= 0; --k) {
    const Fr o = k ? mul(pre[k - 1], J) : J;
    if (k) J = mul(J, v[k]);
    if (lo + k < n) poly_st(out + lo + k, inv_select((zeros >> k) & 1u, o, zero));
  }
}

// ---- host side
// The product tree on one thread, level by level as the workgroup walks it.  s: 2 << log_w nodes, the leaves filled by the caller.
inline void inv_tree_up_host(Fr* s, int log_w) {
  for (int lvl = log_w - 1; lvl >= 0; --lvl)
    for (int i = 1 << lvl; i < 2 << lvl; ++i) s[i] = mul(s[2 * i], s[2 * i + 1]);
}
inline void inv_tree_down_host(Fr* s, int log_w) {   // s[1] holds the inverse of the root's product
  for (int lvl = 0; lvl < log_w; ++lvl)
    for (int i = 1 << lvl; i < 2 << lvl; ++i) {
      const Fr l = s[2 * i], r = s[2 * i + 1];
      s[2 * i] = mul(s[i], r);
      s[2 * i + 1] = mul(s[i], l);
    }
}
// launch 2 on the host: prod[t] (tile products) -> their inverses, INV_CARRY_W at a time, with ONE inv()
inline void inv_carry_host(Fr* prod, size_t n_tiles) {
  const size_t n_chunks = (n_tiles + INV_CARRY_W - 1) / INV_CARRY_W;
  std::vector<Fr> s(2 * INV_CARRY_W), before(n_chunks);
  auto fill = [&](size_t c) {
    for (int l = 0; l < INV_CARRY_W; ++l) {
      const size_t t = c * INV_CARRY_W + l;
      s[INV_CARRY_W + l] = t < n_tiles ? prod[t] : Fr::one();
    }
    inv_tree_up_host(s.data(), INV_LOG_CARRY);
  };
  Fr carry = Fr::one();
  for (size_t c = 0; c < n_chunks; ++c) {   // going up: the product of everything before the chunk
    fill(c);
    before[c] = carry;
    carry = mul(carry, s[1]);
  }
  Fr J = inv(carry);
  for (size_t c = n_chunks; c-- > 0;) {     // coming down: J = (chunks 0 .. c)^-1
    if (c + 1 != n_chunks) fill(c);         // (the last chunk's tree is still there)
    const Fr chunk = s[1];
    s[1] = mul(J, before[c]);
    inv_tree_down_host(s.data(), INV_LOG_CARRY);
    for (int l = 0; l < INV_CARRY_W; ++l)
      if (c * INV_CARRY_W + l < n_tiles) prod[c * INV_CARRY_W + l] = s[INV_CARRY_W + l];
    J = mul(J, chunk);
  }
}
// The whole call on the host, in the kernels' grouping (three launches, or one when INV_ONE_LAUNCH).  out may be in.  Returns the number of zeros.
inline uint32_t inv_batch_host(Fr* out, const Fr* in, size_t n) {
  const size_t n_tiles = (n + INV_TILE - 1) / INV_TILE;
  std::vector<Fr> tinv(n_tiles), s(2 * INV_WG);
  Fr v[INV_RUN];
  uint32_t n_zero = 0;
  if (!INV_ONE_LAUNCH) {
    for (size_t t = 0; t < n_tiles; ++t) {   // launch 1
      for (int l = 0; l < INV_WG; ++l) {
        const uint32_t zeros = inv_run_load(v, in, (t * INV_WG + l) * INV_RUN, n);
        n_zero += (uint32_t)__builtin_popcount(zeros);
        s[INV_WG + l] = inv_run_product(v);
      }
      inv_tree_up_host(s.data(), INV_LOG_WG);
      tinv[t] = s[1];
    }
    inv_carry_host(tinv.data(), n_tiles);    // launch 2
  }
  std::vector<uint32_t> zeros(INV_WG);
  std::vector<Fr> vs((size_t)INV_WG * INV_RUN), pres((size_t)INV_WG * INV_RUN);
  for (size_t t = 0; t < n_tiles; ++t) {     // launch 3 (the only one of variant (b))
    for (int l = 0; l < INV_WG; ++l) {       // every lane loads before any lane stores: out may be in
      zeros[l] = inv_run_load(&vs[(size_t)l * INV_RUN], in, (t * INV_WG + l) * INV_RUN, n);
      if (INV_ONE_LAUNCH) n_zero += (uint32_t)__builtin_popcount(zeros[l]);
      inv_run_prefix(&pres[(size_t)l * INV_RUN], &vs[(size_t)l * INV_RUN]);
      s[INV_WG + l] = pres[(size_t)l * INV_RUN + INV_RUN - 1];
    }
    inv_tree_up_host(s.data(), INV_LOG_WG);
    s[1] = INV_ONE_LAUNCH ? inv(s[1]) : tinv[t];
    inv_tree_down_host(s.data(), INV_LOG_WG);
    for (int l = 0; l < INV_WG; ++l)
      inv_run_apply(out, &vs[(size_t)l * INV_RUN], &pres[(size_t)l * INV_RUN], zeros[l], (t * INV_WG + l) * INV_RUN, n, s[INV_WG + l]);
  }
  return n_zero;
}

#if defined(__HIPCC__)
// fr_inverse.hip, for the other units of the library: `rows` vectors of n elements, row r at d_io + r * stride, inverted IN PLACE with one
// Fermat inversion for all of them (what lies between two rows is neither read nor written).  n < 2^32, rows <= 65535.  Enqueued on `st`.
// d_n_zero: NULL, or a device counter (cleared by the caller) that the zeros of all the rows are added to.
int fr_inverse_rows(Fr* d_io, size_t n, size_t stride, size_t rows, hipStream_t st, uint32_t* d_n_zero = nullptr);
#endif

}  // namespace zk
