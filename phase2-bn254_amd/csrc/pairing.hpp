// The BN254 optimal ate pairing, stated once for device and host: the tower Fq6 = Fq2[v]/(v^3 - xi), Fq12 = Fq6[w]/(w^2 - v) over the
// Fq2 of field.hpp (xi = 9 + u), the Miller loop over 6u + 2 with T in homogeneous projective coordinates on the D-type twist
// y^2 = x^3 + 3 / xi, and the final exponentiation by (q^12 - 1) / r.  The kernels of pairing.hip, the host product
// mi355zk_bn254_pairing_product and the self-test hook all run this text.
//
// What the reference computes (pairing/src/bn256/mod.rs:57-226): Engine::miller_loop over prepared coefficients, then
// final_exponentiation.  Here there is no coefficient array: each line is produced by a doubling or addition step and multiplied into f at
// once (a 0-3-4 sparse product after scaling by P.y and P.x).  The Miller value itself differs from the reference's by factors of the
// proper subfield Fq2 -- other coordinates for T, other scalings of the lines, another signed-digit form of 6u + 2 -- and the final
// exponentiation, whose exponent contains q^6 - 1, removes every such factor: the GT value is the unique r-th root of unity
// e(P, Q)^((q^12 - 1) / r), fully reduced, and its 384 bytes are the reference's (into_raw_repr of each of the twelve Fq, in the order
// c0.c0.c0, c0.c0.c1, c0.c1.c0, ..., c1.c2.c1: Fq12 -> Fq6 -> Fq2 -> Fq).
//
// DOMAIN.  Points are raw affine records (64 B G1, 128 B G2, Montgomery limbs), the all-zero record is the point at infinity and a pair
// with one contributes the value one (mod.rs:68).  P lies on y^2 = x^3 + 3, Q on the twist AND in its order-r subgroup; the reference
// tests neither (G2Prepared::from_affine takes what it is given), and neither does this code: callers holding untrusted G2 points run
// mi355zk_bn254_g2_subgroup_check_dev first.  Outside the domain the result is unspecified; nothing faults -- every step is straight-line
// field arithmetic on registers and private memory, no address and no trip count depends on the data.
//
// NO EXCEPTIONAL BRANCH IN THE LINE FORMULAS.  For Q of prime order r the point T before a step is m Q with m a proper prefix of the
// signed-digit form of 6u + 2, 1 < m < 2^65 < r, so T is neither infinity (the doubling step's only degenerate input, Y = 0, is a point of
// order two) nor +-Q (m = +-1 mod r), which is all the addition step needs: it adds +-Q.  The two closing additions add pi(Q) = q Q and
// -pi^2(Q) = -q^2 Q (on the trace-zero subgroup the Frobenius is multiplication by q) to (6u + 2) Q and (6u + 2 + q) Q; neither of
// 6u + 2 -+ q and 6u + 2 + q -+ q^2 vanishes mod r -- the last one is -q^3, the sum the optimal ate pairing is built on.
// tools/gen_pairing_constants.py checks each of these congruences when it writes the constants.
//
// REGISTERS.  One Fq12 is 96 VGPRs, so nothing above Fq2 lives in registers: Fq6 and Fq12 routines work on references, one Fq2
// coefficient at a time, and are NOT inlined (ZK_HDN) -- a kernel is a call tree over the few Fq2 routines that contain the inline-assembly
// products, its Fq12 values live in private memory, and no coefficient is reached through a runtime index.  The resource figures of
// each kernel are in profiles/pairing.md.
#pragma once

#include "curve.hpp"

#if defined(__HIPCC__)
#define ZK_HDN inline __host__ __device__ __noinline__
#else
#define ZK_HDN inline __attribute__((noinline))
#endif

namespace zk {

#include "pairing_constants.inc"

struct Fq6 {
  Fq2 c0, c1, c2;
};
struct Fq12 {
  Fq6 c0, c1;
};
struct G2Proj {  // homogeneous projective: x = X / Z, y = Y / Z
  Fq2 x, y, z;
};
static_assert(sizeof(Fq12) == 384 && sizeof(Fq6) == 192, "the GT format is the struct");

#define ZK_PAIRING_FQ2_CONST(fn, NAME)       \
  ZK_HD Fq2 fn() {                           \
    Fq2 r;                                   \
    _Pragma("unroll") for (int i = 0; i < 8; ++i) { \
      r.c0.l[i] = PairingConst::NAME[i];     \
      r.c1.l[i] = PairingConst::NAME[8 + i]; \
    }                                        \
    return r;                                \
  }
ZK_PAIRING_FQ2_CONST(pc_twist_b, TWIST_B)
ZK_PAIRING_FQ2_CONST(pc_twist_frob_y, TWIST_FROB_Y)
ZK_PAIRING_FQ2_CONST(pc_frob6_c1_1, FROB6_C1_1)
ZK_PAIRING_FQ2_CONST(pc_frob6_c1_2, FROB6_C1_2)
ZK_PAIRING_FQ2_CONST(pc_frob6_c1_3, FROB6_C1_3)
ZK_PAIRING_FQ2_CONST(pc_frob6_c2_1, FROB6_C2_1)
ZK_PAIRING_FQ2_CONST(pc_frob6_c2_2, FROB6_C2_2)
ZK_PAIRING_FQ2_CONST(pc_frob6_c2_3, FROB6_C2_3)
ZK_PAIRING_FQ2_CONST(pc_frob12_c1_1, FROB12_C1_1)
ZK_PAIRING_FQ2_CONST(pc_frob12_c1_2, FROB12_C1_2)
ZK_PAIRING_FQ2_CONST(pc_frob12_c1_3, FROB12_C1_3)
#undef ZK_PAIRING_FQ2_CONST
ZK_HD Fq pc_two_inv() {
  Fq r;
#pragma unroll
  for (int i = 0; i < 8; ++i) r.l[i] = PairingConst::TWO_INV[i];
  return r;
}

// ---- Fq2: the routines that hold the products (not inlined: every caller above is a handful of calls), and the cheap inline rest.
// Every routine below computes into locals and writes its result last: the result may alias an operand.
ZK_HDN void p_mul(Fq2& r, const Fq2& a, const Fq2& b) { r = mul(a, b); }
ZK_HDN void p_sqr(Fq2& r, const Fq2& a) { r = sqr(a); }
ZK_HDN void p_mul_fq(Fq2& r, const Fq2& a, const Fq& s) { r = Fq2{mul(a.c0, s), mul(a.c1, s)}; }
ZK_HDN void p_inv(Fq2& r, const Fq2& a) { r = inv(a); }
ZK_HD Fq2 fq2_conj(const Fq2& a) { return Fq2{a.c0, neg(a.c1)}; }
// xi a = (9 + u)(a0 + a1 u) = (9 a0 - a1) + (9 a1 + a0) u
ZK_HD Fq2 mul_by_xi(const Fq2& a) {
  const Fq2 a8 = dbl(dbl(dbl(a)));
  return Fq2{sub(add(a8.c0, a.c0), a.c1), add(add(a8.c1, a.c1), a.c0)};
}

// ---- Fq6 = Fq2[v] / (v^3 - xi)
ZK_HD Fq6 fq6_zero() { return Fq6{Fq2::zero(), Fq2::zero(), Fq2::zero()}; }
ZK_HD Fq6 fq6_one() { return Fq6{Fq2::one(), Fq2::zero(), Fq2::zero()}; }
ZK_HDN void fq6_add(Fq6& r, const Fq6& a, const Fq6& b) {
  r.c0 = add(a.c0, b.c0);
  r.c1 = add(a.c1, b.c1);
  r.c2 = add(a.c2, b.c2);
}
ZK_HDN void fq6_sub(Fq6& r, const Fq6& a, const Fq6& b) {
  r.c0 = sub(a.c0, b.c0);
  r.c1 = sub(a.c1, b.c1);
  r.c2 = sub(a.c2, b.c2);
}
ZK_HDN void fq6_neg(Fq6& r, const Fq6& a) {
  r.c0 = neg(a.c0);
  r.c1 = neg(a.c1);
  r.c2 = neg(a.c2);
}
// v (c0 + c1 v + c2 v^2) = xi c2 + c0 v + c1 v^2: multiplication by the non-residue of Fq12 over Fq6
ZK_HDN void fq6_mul_by_nonresidue(Fq6& r, const Fq6& a) {
  const Fq2 t = mul_by_xi(a.c2);
  r.c2 = a.c1;
  r.c1 = a.c0;
  r.c0 = t;
}
// Karatsuba over the three coefficients: 6 Fq2 products
ZK_HDN void fq6_mul(Fq6& r, const Fq6& a, const Fq6& b) {
  Fq2 aa, bb, cc, t, c0, c1;
  p_mul(aa, a.c0, b.c0);
  p_mul(bb, a.c1, b.c1);
  p_mul(cc, a.c2, b.c2);
  p_mul(t, add(a.c1, a.c2), add(b.c1, b.c2));
  c0 = add(aa, mul_by_xi(sub(sub(t, bb), cc)));
  p_mul(t, add(a.c0, a.c1), add(b.c0, b.c1));
  c1 = add(sub(sub(t, aa), bb), mul_by_xi(cc));
  p_mul(t, add(a.c0, a.c2), add(b.c0, b.c2));
  r.c2 = add(sub(sub(t, aa), cc), bb);
  r.c0 = c0;
  r.c1 = c1;
}
// a * s for s in Fq2
ZK_HDN void fq6_scale(Fq6& r, const Fq6& a, const Fq2& s) {
  p_mul(r.c0, a.c0, s);
  p_mul(r.c1, a.c1, s);
  p_mul(r.c2, a.c2, s);
}
// a * (b0 + b1 v): 5 products
ZK_HDN void fq6_mul_by_01(Fq6& r, const Fq6& a, const Fq2& b0, const Fq2& b1) {
  Fq2 aa, bb, t, c0, c1;
  p_mul(aa, a.c0, b0);
  p_mul(bb, a.c1, b1);
  p_mul(t, add(a.c1, a.c2), b1);
  c0 = add(aa, mul_by_xi(sub(t, bb)));
  p_mul(t, add(a.c0, a.c1), add(b0, b1));
  c1 = sub(sub(t, aa), bb);
  p_mul(t, add(a.c0, a.c2), b0);
  r.c2 = add(sub(t, aa), bb);
  r.c0 = c0;
  r.c1 = c1;
}
// a * (b1 v): 3 products
ZK_HDN void fq6_mul_by_1(Fq6& r, const Fq6& a, const Fq2& b1) {
  Fq2 t0, t1, t2;
  p_mul(t0, a.c2, b1);
  p_mul(t1, a.c0, b1);
  p_mul(t2, a.c1, b1);
  r.c0 = mul_by_xi(t0);
  r.c1 = t1;
  r.c2 = t2;
}
// 1 / a through the cofactors and the norm to Fq2; the inverse of zero is zero
ZK_HDN void fq6_inv(Fq6& r, const Fq6& a) {
  Fq2 c0, c1, c2, t, s;
  p_sqr(c0, a.c0);
  p_mul(t, a.c1, a.c2);
  c0 = sub(c0, mul_by_xi(t));            // a0^2 - xi a1 a2
  p_sqr(c1, a.c2);
  p_mul(t, a.c0, a.c1);
  c1 = sub(mul_by_xi(c1), t);            // xi a2^2 - a0 a1
  p_sqr(c2, a.c1);
  p_mul(t, a.c0, a.c2);
  c2 = sub(c2, t);                       // a1^2 - a0 a2
  p_mul(t, a.c2, c1);
  p_mul(s, a.c1, c2);
  t = mul_by_xi(add(t, s));
  p_mul(s, a.c0, c0);
  p_inv(t, add(t, s));                   // 1 / (a0 c0 + xi (a2 c1 + a1 c2))
  p_mul(r.c0, c0, t);
  p_mul(r.c1, c1, t);
  p_mul(r.c2, c2, t);
}
// a^(q^k), k = 1, 2, 3: conjugate the coefficients for odd k, then v -> xi^((q^k - 1) / 3) v
ZK_HDN void fq6_frobenius_map(Fq6& r, const Fq6& a, int k) {
  const bool odd = k & 1;
  r.c0 = odd ? fq2_conj(a.c0) : a.c0;
  p_mul(r.c1, odd ? fq2_conj(a.c1) : a.c1, k == 1 ? pc_frob6_c1_1() : k == 2 ? pc_frob6_c1_2() : pc_frob6_c1_3());
  p_mul(r.c2, odd ? fq2_conj(a.c2) : a.c2, k == 1 ? pc_frob6_c2_1() : k == 2 ? pc_frob6_c2_2() : pc_frob6_c2_3());
}

// ---- Fq12 = Fq6[w] / (w^2 - v)
ZK_HD Fq12 fq12_one() { return Fq12{fq6_one(), fq6_zero()}; }
ZK_HDN void fq12_mul(Fq12& r, const Fq12& a, const Fq12& b) {
  Fq6 aa, bb, t, s;
  fq6_mul(aa, a.c0, b.c0);
  fq6_mul(bb, a.c1, b.c1);
  fq6_add(t, a.c0, a.c1);
  fq6_add(s, b.c0, b.c1);
  fq6_mul(t, t, s);
  fq6_sub(t, t, aa);
  fq6_sub(r.c1, t, bb);
  fq6_mul_by_nonresidue(bb, bb);
  fq6_add(r.c0, aa, bb);
}
// (a0 + a1 w)^2 = (a0 + a1)(a0 + v a1) - a0 a1 - v a0 a1 + 2 a0 a1 w: 2 Fq6 products
ZK_HDN void fq12_sqr(Fq12& r, const Fq12& a) {
  Fq6 ab, t, s;
  fq6_mul(ab, a.c0, a.c1);
  fq6_add(t, a.c0, a.c1);
  fq6_mul_by_nonresidue(s, a.c1);
  fq6_add(s, s, a.c0);
  fq6_mul(t, t, s);
  fq6_sub(t, t, ab);
  fq6_mul_by_nonresidue(s, ab);
  fq6_sub(r.c0, t, s);
  fq6_add(r.c1, ab, ab);
}
// 1 / (a0 + a1 w) = (a0 - a1 w) / (a0^2 - v a1^2); the inverse of zero is zero
ZK_HDN void fq12_inv(Fq12& r, const Fq12& a) {
  Fq6 t, s;
  fq6_mul(t, a.c0, a.c0);
  fq6_mul(s, a.c1, a.c1);
  fq6_mul_by_nonresidue(s, s);
  fq6_sub(t, t, s);
  fq6_inv(t, t);
  fq6_mul(r.c0, a.c0, t);
  fq6_mul(s, a.c1, t);
  fq6_neg(r.c1, s);
}
// a^(q^6)
ZK_HDN void fq12_conjugate(Fq12& r, const Fq12& a) {
  r.c0 = a.c0;
  fq6_neg(r.c1, a.c1);
}
// a^(q^k), k = 1, 2, 3: both halves through fq6_frobenius_map, then w -> xi^((q^k - 1) / 6) w
ZK_HDN void fq12_frobenius_map(Fq12& r, const Fq12& a, int k) {
  fq6_frobenius_map(r.c0, a.c0, k);
  fq6_frobenius_map(r.c1, a.c1, k);
  fq6_scale(r.c1, r.c1, k == 1 ? pc_frob12_c1_1() : k == 2 ? pc_frob12_c1_2() : pc_frob12_c1_3());
}
// f *= c0 + (c3 + c4 v) w, the shape of a line on the D-type twist: 13 Fq2 products instead of 18
ZK_HDN void fq12_mul_by_034(Fq12& f, const Fq2& c0, const Fq2& c3, const Fq2& c4) {
  Fq6 a, b, e;
  fq6_scale(a, f.c0, c0);
  fq6_mul_by_01(b, f.c1, c3, c4);
  fq6_add(e, f.c0, f.c1);
  fq6_mul_by_01(e, e, add(c0, c3), c4);
  fq6_sub(e, e, a);
  fq6_sub(f.c1, e, b);
  fq6_mul_by_nonresidue(b, b);
  fq6_add(f.c0, a, b);
}

// ---- the Miller loop.  A step moves T and leaves the line through the points it combined, as the three coefficients (l0, l3, l4) of
// l0 y_P + l3 x_P w + l4 v w  (the untwist sends (x', y') to (x' w^2, y' w^3); a line is determined up to a factor in Fq2).
// T = 2 T for Y^2 Z = X^3 + b' Z^3; the tangent at T scaled by -2 Y Z:  (-2 Y Z, 3 X^2, 3 b' Z^2 - Y^2)
ZK_HDN void pairing_double_step(G2Proj& t, Fq2& l0, Fq2& l3, Fq2& l4) {
  Fq2 a, b, c, e, f, g, h, j, s;
  p_mul(a, t.x, t.y);
  p_mul_fq(a, a, pc_two_inv());          // X Y / 2
  p_sqr(b, t.y);
  p_sqr(c, t.z);
  p_mul(e, pc_twist_b(), add(dbl(c), c));   // 3 b' Z^2
  f = add(dbl(e), e);                       // 9 b' Z^2
  p_mul_fq(g, add(b, f), pc_two_inv());
  p_sqr(h, add(t.y, t.z));
  h = sub(h, add(b, c));                    // 2 Y Z
  p_sqr(j, t.x);
  l0 = neg(h);
  l3 = add(dbl(j), j);
  l4 = sub(e, b);
  p_mul(t.x, a, sub(b, f));
  p_sqr(s, e);
  p_sqr(g, g);
  t.y = sub(g, add(dbl(s), s));             // ((Y^2 + 9 b' Z^2) / 2)^2 - 3 (3 b' Z^2)^2
  p_mul(t.z, b, h);
}
// T = T + Q for an affine Q != +-T; with theta = Y - y_Q Z, lambda = X - x_Q Z the chord scaled by lambda:  (lambda, -theta, theta x_Q - lambda y_Q)
ZK_HDN void pairing_add_step(G2Proj& t, const Fq2& qx, const Fq2& qy, Fq2& l0, Fq2& l3, Fq2& l4) {
  Fq2 theta, lambda, c, d, e, f, g, h, s;
  p_mul(s, qy, t.z);
  theta = sub(t.y, s);
  p_mul(s, qx, t.z);
  lambda = sub(t.x, s);
  p_sqr(c, theta);
  p_sqr(d, lambda);
  p_mul(e, lambda, d);
  p_mul(f, t.z, c);
  p_mul(g, t.x, d);
  h = sub(add(e, f), dbl(g));
  p_mul(t.x, lambda, h);
  p_mul(s, theta, sub(g, h));
  p_mul(c, e, t.y);
  t.y = sub(s, c);
  p_mul(t.z, t.z, e);
  p_mul(s, theta, qx);
  p_mul(c, lambda, qy);
  l0 = lambda;
  l3 = neg(theta);
  l4 = sub(s, c);
}
// f *= the line at P
ZK_HDN void pairing_ell(Fq12& f, Fq2& l0, Fq2& l3, const Fq2& l4, const Affine<Fq>& p) {
  p_mul_fq(l0, l0, p.y);
  p_mul_fq(l3, l3, p.x);
  fq12_mul_by_034(f, l0, l3, l4);
}

// f = the Miller value of one pair (one if either point is the all-zero record)
ZK_HDN void pairing_miller_loop(Fq12& f, const Affine<Fq>& p, const Affine<Fq2>& q) {
  f = fq12_one();
  if (p.is_zero() || q.is_zero()) return;
  G2Proj t{q.x, q.y, Fq2::one()};
  const Fq2 neg_qy = neg(q.y);
  Fq2 l0, l3, l4;
#pragma unroll 1
  for (int i = 63; i >= 0; --i) {          // digit 64 of the signed-digit form is the leading 1: T = Q, f = 1
    if (i != 63) fq12_sqr(f, f);
    pairing_double_step(t, l0, l3, l4);
    pairing_ell(f, l0, l3, l4, p);
    const bool pos = (PairingConst::ATE_NAF_POS >> i) & 1u, minus = (PairingConst::ATE_NAF_NEG >> i) & 1u;
    if (pos || minus) {
      pairing_add_step(t, q.x, minus ? neg_qy : q.y, l0, l3, l4);
      pairing_ell(f, l0, l3, l4, p);
    }
  }
  Fq2 x1, y1;
  p_mul(x1, fq2_conj(q.x), pc_frob6_c1_1());   // pi(Q)
  p_mul(y1, fq2_conj(q.y), pc_twist_frob_y());
  pairing_add_step(t, x1, y1, l0, l3, l4);
  pairing_ell(f, l0, l3, l4, p);
  p_mul(x1, q.x, pc_frob6_c1_2());             // -pi^2(Q): the y factor of pi^2 is xi^((q^2 - 1) / 2) = -1
  pairing_add_step(t, x1, q.y, l0, l3, l4);
  pairing_ell(f, l0, l3, l4, p);
}

// r = a^u by square-and-multiply over the 63 bits of u (r must not alias a)
ZK_HDN void pairing_exp_by_u(Fq12& r, const Fq12& a) {
  r = a;
#pragma unroll 1
  for (int i = 61; i >= 0; --i) {
    fq12_sqr(r, r);
    if ((PairingConst::BN_U >> i) & 1u) fq12_mul(r, r, a);
  }
}
static_assert((PairingConst::BN_U >> 62) == 1, "the loop of pairing_exp_by_u starts below bit 62");

// f^((q^12 - 1) / r) = (f^((q^6 - 1)(q^2 + 1)))^((q^4 - q^2 + 1) / r).  The hard exponent is EXACTLY
//   q^3 + (6u^2 + 1) q^2 + (-36u^3 - 18u^2 - 12u + 1) q + (-36u^3 - 30u^2 - 18u - 2)
// (Scott, Benger, Charlemagne, Dominguez Perez, Kachisa, "On the final exponentiation for calculating pairings on ordinary elliptic
// curves"), evaluated as y0 y1^2 y2^6 y3^12 y4^18 y5^30 y6^36 over three powers by u, as the reference does (mod.rs:148-222), so the
// bytes agree.  After the easy part the value is unitary: its inverse is its conjugate.  A zero input (never a Miller value) gives zero.
ZK_HDN void pairing_final_exponentiation(Fq12& out, const Fq12& f) {
  Fq12 r, fu, fu2, fu3, t0, t1, s;
  fq12_conjugate(t0, f);
  fq12_inv(t1, f);
  fq12_mul(t0, t0, t1);                  // f^(q^6 - 1)
  fq12_frobenius_map(r, t0, 2);
  fq12_mul(r, r, t0);                    // ... ^(q^2 + 1)
  pairing_exp_by_u(fu, r);
  pairing_exp_by_u(fu2, fu);
  pairing_exp_by_u(fu3, fu2);
  fq12_frobenius_map(s, fu3, 1);
  fq12_mul(t0, fu3, s);
  fq12_conjugate(t0, t0);                // y6 = 1 / (f^(u^3) f^(u^3 q))
  fq12_sqr(t0, t0);
  fq12_frobenius_map(s, fu2, 1);
  fq12_mul(s, s, fu);
  fq12_conjugate(s, s);                  // y4 = 1 / (f^u f^(u^2 q))
  fq12_mul(t0, t0, s);
  fq12_conjugate(fu3, fu2);              // y5 = 1 / f^(u^2)
  fq12_mul(t0, t0, fu3);                 // T0 = y6^2 y4 y5
  fq12_frobenius_map(s, fu, 1);
  fq12_conjugate(s, s);                  // y3 = 1 / f^(u q)
  fq12_mul(t1, s, fu3);
  fq12_mul(t1, t1, t0);                  // T1 = y3 y5 T0
  fq12_frobenius_map(s, fu2, 2);         // y2 = f^(u^2 q^2)
  fq12_mul(t0, t0, s);
  fq12_sqr(t1, t1);
  fq12_mul(t1, t1, t0);
  fq12_sqr(t1, t1);
  fq12_conjugate(s, r);                  // y1 = 1 / f
  fq12_mul(t0, t1, s);
  fq12_frobenius_map(s, r, 1);
  fq12_frobenius_map(fu, r, 2);
  fq12_mul(s, s, fu);
  fq12_frobenius_map(fu, r, 3);
  fq12_mul(s, s, fu);                    // y0 = f^q f^(q^2) f^(q^3)
  fq12_mul(t1, t1, s);
  fq12_sqr(t0, t0);
  fq12_mul(out, t0, t1);
}

}  // namespace zk
