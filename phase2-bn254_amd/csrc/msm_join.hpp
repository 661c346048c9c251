#pragma once
// The host join that ends a multiexp (msm_host.hpp: msm_device): the WL * n_out partial sums the device hands back, each carrying a
// power of two (and of the radix), become one group element.  Host arithmetic only -- no HIP call -- so that it is tested without a
// device (tests/test_msm_join_host.py).
#include <vector>

#include "curve.hpp"
#include "host_util.hpp"
#include "msm_plan.hpp"

namespace zk {

namespace {

// R-domain record -> Jacobian in the memory format, for the host join.  The record's limbs, READ in the memory format's 2^256
// domain, are the coordinates times f = 2^5 -- all four by the same f -- and  x = X / ZZ,  y = Y / ZZZ  do not see a common factor
// (which is why xyzz_to_affine takes a record as it is).  A Jacobian triple with the same property, for ANY such quadruple:
//     z = ZZ * ZZZ,   x_j = X * ZZ * ZZZ^2,   y_j = Y * ZZ^3 * ZZZ^2        (x_j / z^2 = X / ZZ,  y_j / z^3 = Y / ZZZ)
// -- 6 products + 2 squarings on the host's 4 x 64-bit Montgomery arithmetic, instead of xyzzr_to_std's four U-form products (plain
// C on nine 29-bit limbs: ~4 x slower per product on a CPU) followed by xyzz_to_jacobian's four: the ~200 window sums of a
// multiexp cost 143 -> ~90 us to join (G2: three times that).
template <class F>
inline Jacobian<F> rec_to_jacobian(const XYZZ<F>& r) {
  if (r.is_zero()) return Jacobian<F>::zero();
  const F t = sqr(r.zzz);
  Jacobian<F> j;
  j.z = mul(r.zz, r.zzz);
  j.x = mul(mul(r.x, r.zz), t);
  j.y = mul(mul(r.y, mul(sqr(r.zz), r.zz)), t);
  return j;
}

template <class F>
inline Jacobian<F> horner(const std::vector<Jacobian<F>>& by_exp) {  // sum_t 2^t by_exp[t]
  Jacobian<F> acc = by_exp.back();
  for (int t = (int)by_exp.size() - 2; t >= 0; --t) {
    jac_double(acc);
    if (!by_exp[t].is_zero()) jac_add(acc, by_exp[t]);
  }
  return acc;
}

// What the join reads of the plan, COPIED out of it: the per-window loops below store field limbs (uint32_t) and read the counts
// and exponents in between.  MEASURED: reading them (and MsmGeom) through the `const MsmPlan&` made the G2 join 10 % slower than with
// these copies (176 -> 195 us at 2^12 .. 2^16, same box, interleaved: profiles/msm_host_split.md section 4) -- presumably because a limb
// store may alias what a reference points to (MsmGeom::shift is bytes) and cannot alias a local of the joining function.
struct JoinTerms {
  uint32_t n_out, e_max;
  uint32_t e_k[MSM_MAX_JOBS];
};

// the n_out partial sums of bucket set wl, collected by their power of two: by_exp[shift + e_k] += P[wl][k]
template <class F>
inline void collect_window(const JoinTerms& J, const XYZZ<F>* h_wsums, uint32_t wl, uint32_t shift, std::vector<Jacobian<F>>& by_exp) {
  const uint32_t n_out = J.n_out;
  for (uint32_t k = 0; k < n_out; ++k) {
    const XYZZ<F>& pt = h_wsums[(size_t)wl * n_out + k];
    if (!pt.is_zero()) jac_add(by_exp[shift + J.e_k[k]], rec_to_jacobian(pt));
  }
}

// T_wl = sum_k 2^e_k P[wl][k]
template <class F>
inline Jacobian<F> window_sum(const JoinTerms& J, const XYZZ<F>* h_wsums, uint32_t wl) {
  std::vector<Jacobian<F>> by_exp((size_t)J.e_max + 1, Jacobian<F>::zero());
  collect_window(J, h_wsums, wl, 0, by_exp);
  return horner(by_exp);
}

// the helper threads of this unit's joins: the window sums of one call, or whole vectors of a batch (msm_join_batch)
inline JoinPool& msm_join_pool() {
  static JoinPool pool;
  return pool;
}

// *result = sum_w 2^shift_w * T_w,  T_w = A_0 + L_0*(A_1 + L_1*(... + sum_j 2^j Bits_j)):  every partial sum
// P[w][k] carries a power of two 2^(shift_w + e_k).  Terms are collected per exponent and ONE Horner pass
// (a doubling per bit, multiexp.rs:146-154) joins everything -- ~270 doublings instead of W * (c + e_max).
// h_wsums: WL * P.n_out records, window-major.  serial: never the helper threads (MsmKnobs::join_serial).
// ran_parallel (tests): whether the helper threads took the window sums.
// WL: the bucket sets joined -- P.WL for a single call; P.WD for ONE vector of a batch, whose records are the slice
// h_wsums + v * P.WD * P.n_out of what came back (the plan's WL counts every vector's sets).
template <class F>
void msm_join(const MsmPlan& P, uint32_t WL, const XYZZ<F>* h_wsums, bool serial, Jacobian<F>* result, bool* ran_parallel = nullptr) {
  const MsmGeom G = P.G;   // (a copy, like J: see JoinTerms)
  const uint32_t w_lo = P.w_lo, w_hi = P.w_hi;
  const bool tmode = P.tmode;
  JoinTerms J;
  J.n_out = P.n_out;
  J.e_max = P.e_max;
  for (uint32_t k = 0; k < P.n_out; ++k) J.e_k[k] = P.e_k[k];
  // The window sums T_w are independent: with the helper threads free (JoinPool: a single caller -- the prover's eight
  // concurrent joins take the single-threaded paths below instead), every T_w is joined from its n_out terms in parallel and
  // only the chain over the windows stays serial: G2 at 2^20 0.48 -> 0.26 ms of host time, G1 0.13 -> 0.08 ms.
  std::vector<Jacobian<F>> T(WL);
  const bool parallel = !serial && WL >= 4 && msm_join_pool().run(WL, [&](uint32_t wl) { T[wl] = window_sum(J, h_wsums, wl); });
  if (ran_parallel) *ran_parallel = parallel;
  Jacobian<F> acc;
  if (parallel && G.rmul == 1) {
    // sum_w 2^shift_w T_w: Horner over the windows from the top one down, then the shift of the group's lowest window
    acc = T[WL - 1];
    for (int wl = (int)WL - 2; wl >= 0; --wl) {
      for (uint32_t r = G.shift[w_lo + wl]; r < G.shift[w_lo + wl + 1]; ++r) jac_double(acc);
      if (!T[wl].is_zero()) jac_add(acc, T[wl]);
    }
    for (uint32_t r = 0; r < G.shift[w_lo]; ++r) jac_double(acc);
  } else if (G.rmul == 1) {
    auto wshift = [&](uint32_t w) -> uint32_t { return tmode ? 0u : G.shift[w]; };  // (table mode: the table carries the shifts)
    std::vector<Jacobian<F>> by_exp((size_t)wshift(w_lo + WL - 1) + J.e_max + 1, Jacobian<F>::zero());
    for (uint32_t wl = 0; wl < WL; ++wl) collect_window(J, h_wsums, wl, wshift(w_lo + wl), by_exp);
    acc = horner(by_exp);
  } else {
    // mixed radix: T_w by its own Horner pass, then  acc = B * acc + T_w  with  B = rmul * 2^rshift; the windows below this
    // call's group contribute nothing here, only their powers of B
    acc = Jacobian<F>::zero();
    for (int w = (int)w_hi - 1; w >= 0; --w) {
      const Jacobian<F> one_acc = acc;            // rmul * acc by double-and-add over the bits of rmul (<= 15)
      int top = 3;
      while (!((G.rmul >> top) & 1u)) --top;
      for (int bit = top - 1; bit >= 0; --bit) {
        jac_double(acc);
        if ((G.rmul >> bit) & 1u) jac_add(acc, one_acc);
      }
      for (uint32_t r = 0; r < G.rshift; ++r) jac_double(acc);
      if (w < (int)w_lo) continue;
      jac_add(acc, parallel ? T[w - (int)w_lo] : window_sum(J, h_wsums, (uint32_t)(w - (int)w_lo)));
    }
  }
  *result = acc;
}
template <class F>
void msm_join(const MsmPlan& P, const XYZZ<F>* h_wsums, bool serial, Jacobian<F>* result, bool* ran_parallel = nullptr) {
  msm_join<F>(P, P.WL, h_wsums, serial, result, ran_parallel);
}

// The joins of a batch: vector v from its WD * n_out records.  The vectors are independent, so with the helper threads free each takes
// whole vectors (a G2 join is ~0.27 ms of host time: sixteen in a row would eat what the batch saves); otherwise -- the prover's eight
// concurrent calls -- one after the other on the caller.
template <class F>
void msm_join_batch(const MsmPlan& P, const XYZZ<F>* h_wsums, uint32_t n_vectors, bool serial, Jacobian<F>* results, bool* ran_parallel = nullptr) {
  const size_t per = (size_t)P.WD * P.n_out;
  auto one = [&](uint32_t v) { msm_join<F>(P, P.WD, h_wsums + v * per, true, &results[v]); };
  const bool parallel = !serial && n_vectors >= 2 && msm_join_pool().run(n_vectors, one);
  if (ran_parallel) *ran_parallel = parallel;
  if (!parallel) for (uint32_t v = 0; v < n_vectors; ++v) one(v);
}

}  // namespace

}  // namespace zk
