// The per-element ARITHMETIC of an Fr transform pass, stated once: the butterfly, the products at a tile's load and store, the closing
// reductions, the element lines of the scale kernel and of the full-table builders -- and the SCHEDULE decisions the bounds hang on (which
// stages may skip a twiddle-one product, when a sum is carried, the constant of a skipped stage's subtraction).  ntt.hip keeps the index,
// LDS, table-address and barrier code and calls these; the host bound checker (tests/cpp/test_ntt_bounds_host.cpp) instantiates the same
// lines on limbs that carry worst-case intervals (tests/cpp/u_interval.hpp) and derives, stage by stage, what the comments below claim.
//
// The chain (printed by the checker: profiles/ntt_bounds.md).  Data is U-form (fieldu.hpp) and is never reduced between stages:
//   load      canonical, < p, N-form; a product by a table constant at the load (pre 1, 2, 4) leaves < 2p, N-form
//   stage s   (u, t) -> (u + w t, u + K p - w t).  w t < 2p by the Shoup product: values grow by 2p per stage.  A SKIPPED product
//             (w = 1: stage 0, twiddle index 0 of the stages up to skip_max) leaves t as large as u, so values DOUBLE there: entering
//             stage s <= skip_max + 1 an element is < 2^s * 2p at most, later < 16p + 2 (s - 3) p (skip_max = 2) -- 30p after ten
//             stages, 28p after the twelve of a 2^12 row (skip_max = 1), 2p + 2 s p on the twisted path (no skip anywhere)
//   limbs     a sum adds one multiple of 2^29 per stage and is carried where (s & 3) == 3: limbs entering stage s are
//             < ((s & 3) + 1) * 2^29, at most 4 * 2^29 = 2^31, the limit of the Shoup product; differences leave carried
//   store     one more product (< 160p in, < 2p out) and u_to_std_lt2p, or u_to_std_lt32p of the carried value (< 32p)
#pragma once

#include "fieldu.hpp"

namespace zk {

// a table constant: the PLAIN canonical integer w on nine 29-bit limbs and wq = floor(w * 2^261 / p) (fieldu.hpp: u_mul_shoup)
struct TwU {
  FrU w, q;
};

// x * (the table constant): the value itself (no Montgomery factor), < 2p for x < 160p with limbs < 2^31
ZK_HD FrU tw_mul(const FrU& x, const TwU& t) { return u_mul_shoup(x, t.w, t.q); }

// x * a * (the constant `second()` yields): the second table entry is asked for after the first product, where the kernels load it
template <class L>
ZK_HD FrU tw_mul2(const FrU& x, const TwU& a, L&& second) {
  const FrU y = tw_mul(x, a);
  return tw_mul(y, second());
}

// entry for the plain canonical integer c (8 x 32-bit words)
ZK_HD TwU tw_make(const Fr& c_plain) {
  TwU t;
  t.w = u_from_std(c_plain);
  t.q = u_shoup_quotient<FrParams>(c_plain.l);
  return t;
}

// The schedule of a row of 2^LOG_NP elements.
//   skip_max     twiddle-one products are skipped in stages 0 .. skip_max.  Rows longer than 2^10 give up stage 2: a skipped stage doubles
//                the value bound instead of adding 2p, and 16p + 2 (LOG_NP - 3) p would pass the 32p the closing reduction allows;
//                8p + 2 (LOG_NP - 2) p does not.  Stage 3 is never skipped: 32p + ... is past it for every row that has a stage 3.
//   carry_sum    the sum of stage ST is carried (the difference always is)
//   skip_sub_k   K of a skipped stage's u_sub<K, 1>: the subtrahend is then as large as an element entering the stage, < 2^ST * 2p
template <uint32_t LOG_NP>
struct NttSchedule {
  static constexpr uint32_t skip_max = LOG_NP > 10 ? 1 : 2;
  static constexpr bool may_skip(uint32_t st) { return st <= skip_max; }
  static constexpr bool carry_sum(uint32_t st) { return (st & 3) == 3; }
  static constexpr int skip_sub_k(uint32_t st) { return (st >= 1 && st <= skip_max) ? (2 << st) : 2; }
};

// One butterfly of stage ST on registers: (u, t) -> (u + w t, u - w t); skip: w = 1 and `w` is not read.  `w` is a TwU, or a callable that
// yields one (the radix-2 loop loads its twiddle only where a product is due).
//   in:  u, t with limbs < ((ST & 3) + 1) * 2^29 (< 2^31: the product's limit; < 2^32 - 2^30 - 16: u_sub's), values as in the head of this file
//   out: the sum's limbs grow by 2^29 (carried when the schedule says so) and its value by value(w t); the difference is N-form
// Handed out as a generic lambda with the stage number as an integral_constant, so that a radix-4 kernel calls the butterfly's own body on
// the four registers of a group and not a wrapper around it (with a function in between hipcc schedules the subtraction differently:
// profiles/ntt_bounds.md).
template <class SCH>
static ZK_HD auto ntt_bf_fn() {
  return [](auto stc, FrU& u, FrU& t, const auto& w, bool skip) {
    constexpr uint32_t ST = (uint32_t) decltype(stc)::value;
    if (!skip) {
      if constexpr (std::is_same_v<std::decay_t<decltype(w)>, TwU>) t = tw_mul(t, w);   // < 2p, N
      else t = tw_mul(t, w());
    } else {
      t = u_carry(t);                                                      // as large as u
    }
    FrU sum = u_add(u, t);
    if constexpr (SCH::carry_sum(ST)) sum = u_carry(sum);
    FrU dif;
    constexpr int KS = SCH::skip_sub_k(ST);
    if constexpr (KS != 2) dif = skip ? u_sub<KS, 1>(u, t) : u_sub<2, 1>(u, t);
    else dif = u_sub<2, 1>(u, t);                                          // t < 2p either way (stage 0 skipped: t as loaded)
    u = sum;
    t = dif;
  };
}
template <uint32_t ST, class SCH, class W>
ZK_HD void ntt_bf(FrU& u, FrU& t, const W& w, bool skip) {
#if defined(__clang__)
  [[clang::always_inline]]
#endif
  ntt_bf_fn<SCH>()(std::integral_constant<int, (int)ST>{}, u, t, w, skip);
}

// The same butterfly for a caller that stores the two results where u and t came from instead of keeping them in registers (the radix-2
// loop); t is left holding w t.  Stated a second time because hipcc's code for that loop follows the statement order of its source: built
// on the lambda above, every radix-2 kernel comes out scheduled differently.  The bound checker runs both forms.
template <uint32_t ST, class SCH, class W>
ZK_HD void ntt_bf_to(const FrU& u, FrU& t, const W& w, bool skip, FrU& sum, FrU& dif) {
  if (!skip) {
    if constexpr (std::is_same_v<W, TwU>) t = tw_mul(t, w);
    else t = tw_mul(t, w());
  } else {
    t = u_carry(t);
  }
  sum = u_add(u, t);
  if constexpr (SCH::carry_sum(ST)) sum = u_carry(sum);
  constexpr int KS = SCH::skip_sub_k(ST);
  if constexpr (KS != 2) {
    if (skip) dif = u_sub<KS, 1>(u, t);
    else dif = u_sub<2, 1>(u, t);
  } else {
    dif = u_sub<2, 1>(u, t);
  }
}

// ---- the load side ----
ZK_HD FrU ntt_load(const Fr& a) { return u_from_std(a); }                                       // canonical: < p, N
// pre == 1: distribute_powers, g^i = A[i >> h] * B[i & mask]: two products
template <class L>
ZK_HD FrU ntt_pre1(const FrU& v, const TwU& a, L&& b) { return tw_mul2(v, a, b); }              // < 2p, N
// pre == 2: (g^S)^x, the row position's factor of a folded table set
ZK_HD FrU ntt_pre2(const FrU& v, const TwU& a) { return tw_mul(v, a); }
// pre == 4: g^col, the column's factor where there is no full table (pre == 3 and the row part of pre == 4 sit in the butterfly twiddles)
ZK_HD FrU ntt_pre4(const FrU& v, const TwU& b) { return tw_mul(v, b); }

// N-form value < 2p -> canonical, in the memory format
ZK_HD Fr ntt_reduce_lt2p(const FrU& v) { return u_to_std_lt2p(v); }

// ---- the store side: v as the last stage left it (< 32p, limbs < 2^31) ----
// the first of two (tw_mul != 0, post == 5) or three (post == 2) products; the last one is ntt_store_mul's
ZK_HD FrU ntt_post_mul(const FrU& v, const TwU& a) { return tw_mul(v, a); }
template <class L>
ZK_HD FrU ntt_post_mul2(const FrU& v, const TwU& a, L&& b) { return tw_mul2(v, a, b); }
// the closing product (inter-pass twiddle, post scale) and the reduction to the memory format
ZK_HD Fr ntt_store_mul(const FrU& v, const TwU& w) { return ntt_reduce_lt2p(tw_mul(v, w)); }
// post == 3: nothing to multiply by -- the value is reduced directly
ZK_HD Fr ntt_store_plain(const FrU& v) { return u_to_std_lt32p(u_carry(v)); }

// ---- ntt_scale_kernel: a *= c (c a Montgomery form in the memory format: c * 2^261 first, then the Montgomery product), then *= A * B ----
ZK_HD FrU ntt_scale_const(const FrU& v, const Fr& c) { return u_mul(v, u_mul(u_from_std(c), UPow2<FrParams, 266>::get())); }   // < 2p, N
template <class L>
ZK_HD FrU ntt_scale_pow(const FrU& v, const TwU& a, L&& b) { return tw_mul2(v, a, b); }

// ---- the full-table builders: w^e = A[e >> h] * B[e & mask], further factors, and the entry of the canonical result ----
ZK_HD FrU ntt_tab_product(const TwU& a, const TwU& b) { return tw_mul(a.w, b); }                 // < 2p, N (and so after every further factor)
ZK_HD FrU ntt_tab_factor(const FrU& w, const TwU& a) { return tw_mul(w, a); }
template <class L>
ZK_HD FrU ntt_tab_factor2(const FrU& w, const TwU& a, L&& b) { return tw_mul2(w, a, b); }
ZK_HD TwU ntt_tab_entry(const FrU& w) { return tw_make(u_to_std_lt2p(w)); }                       // canonical, and its quotient

}  // namespace zk
