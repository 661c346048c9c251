// Limbs and column sums that carry a worst-case INTERVAL next to their value: the types csrc/fieldu.hpp computes on when ZK_U_BOUNDS_CHECK
// is defined (there: ulimb_t, uacc_t, UValueBound, UChk).  Include this file INSTEAD of fieldu.hpp / curveu.hpp; it includes curveu.hpp at
// its end, so what runs are the header's own lines, instantiated on these types (tests/cpp/test_u_bounds_host.cpp).
//
// What is tracked
//   IvLimb  a 32-bit limb: the value of one concrete run (it steers the branches) and [lo, hi], the integers the limb can be over ALL
//           inputs inside the stated bounds, NOT reduced mod 2^32.  Sums and differences only widen the interval; whatever CONSUMES a
//           limb as a number (a product, a shift, a mask, the conversion to a column term) reports it if lo < 0 or hi >= 2^32:
//           "limb expression can wrap".  So limbs 0..7 of a lazy subtraction are judged where u_carry or a product reads them.
//   IvAcc   a 64-bit column sum with [lo, hi] on 128 bits; `+=` reports hi >= 2^64: "column sum can exceed 2^64".
//   value   every FpU carries vb: value < vb * p (UValueBound), infinite ("unknown") until some hook sets it.  The hooks of fieldu.hpp (UChk) set it by the RESULT lines stated there
//           (u_mul: < a b / 2^261 + p; u_sub: < a + K p; ...) and test the stated PRECONDITIONS against what the caller passed.
//   limb 8  is correlated with the value: u_sub lets it wrap in u32 arithmetic until the carry, so its interval may reach below zero and
//           is not judged there.  It is judged through the value bound: after the carry the element is N-form and its value is
//           >= 0 (value(b) <= K p was tested) and < vb p, hence l[8] = value >> 232 lies in [0, vb * (p >> 232) + vb) -- `carried_nonneg`
//           REPLACES the interval of limb 8 by that range.  The same holds for a Montgomery result (N-form, 0 <= value < vb p).  An
//           un-carried difference (u_sub_lazy) keeps the plain interval a.l[8] + (K p >> 232) - S - b.l[8]: if that can be negative, the
//           product that reads it reports it.
#pragma once
#define ZK_U_BOUNDS_CHECK 2   // 2: UChk has the hooks of u_mul_shoup, u_mul3 / u_mul4 and u_from_std (fieldu.hpp: UChk2)

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace zk {

struct UViolations {
  std::vector<std::string> list;
  const char* where = "?";
  void add(const std::string& what) {
    std::string s = std::string(where) + ": " + what;
    for (const auto& x : list)
      if (x == s) return;
    list.push_back(s);
  }
};
inline UViolations& u_violations() {
  static UViolations v;
  return v;
}

struct IvAcc;
struct IvLimb {
  uint32_t v;
  int64_t lo, hi;
  bool wide;  // a left shift or a truncation whose mathematical result passes 2^32 ON PURPOSE: only a mask (or the wrapping product of the Montgomery factor) may read it
  IvLimb() : v(0), lo(0), hi(0), wide(false) {}
  IvLimb(uint32_t c) : v(c), lo(c), hi(c), wide(false) {}
  IvLimb(uint32_t c, int64_t l, int64_t h) : v(c), lo(l), hi(h), wide(false) {}
  explicit IvLimb(const IvAcc& a);
  bool fits() const { return lo >= 0 && hi < (int64_t(1) << 32); }
  const IvLimb& read(const char* by) const {
    if (!fits() || wide) u_violations().add(std::string("limb expression can wrap (read by ") + by + "): [" + std::to_string(lo) + ", " + std::to_string(hi) + "]");
    return *this;
  }
  explicit operator uint32_t() const { return read("a conversion to a plain word").v; }
  IvLimb& operator|=(const IvLimb& b);
};
inline int64_t iv_bits_mask(int64_t hi) {
  int64_t m = 1;
  while (m <= hi) m <<= 1;
  return m - 1;
}
// u32 arithmetic is modular: an interval may be moved by 2^32 without changing what it says.  One that lies wholly below -2^31 (the
// `- m` of  (x ^ m) - m  with m = ~0, which takes 2^32 - 1 off the complement -x - 1) is moved up, so that it reads [-x.hi, -x.lo].
inline IvLimb iv_mod(IvLimb r) {
  while (r.hi < -(int64_t(1) << 31)) r.lo += int64_t(1) << 32, r.hi += int64_t(1) << 32;
  return r;
}
inline IvLimb operator+(const IvLimb& a, const IvLimb& b) { return iv_mod(IvLimb(a.v + b.v, a.lo + b.lo, a.hi + b.hi)); }
inline IvLimb operator-(const IvLimb& a, const IvLimb& b) { return iv_mod(IvLimb(a.v - b.v, a.lo - b.hi, a.hi - b.lo)); }
inline IvLimb operator<<(const IvLimb& a, int k) {
  a.read("<<");
  IvLimb r(a.v << k, a.lo << k, a.hi << k);
  r.wide = !r.fits();
  return r;
}
inline IvLimb operator>>(const IvLimb& a, int k) {
  a.read(">>");
  return IvLimb(a.v >> k, a.lo >> k, a.hi >> k);
}
inline IvLimb operator&(const IvLimb& a, const IvLimb& b) {
  // one side is a constant mask 2^k - 1 in every use; the other may be `wide` (truncated on purpose)
  const IvLimb& m = (b.lo == b.hi) ? b : a;
  const IvLimb& x = (b.lo == b.hi) ? a : b;
  if (!x.wide) x.read("&");
  if (x.lo >= 0 && x.hi <= m.hi && !x.wide) return IvLimb(x.v & m.v, x.lo, x.hi);
  return IvLimb(x.v & m.v, 0, m.hi);
}
inline IvLimb operator|(const IvLimb& a, const IvLimb& b) {
  a.read("|"), b.read("|");
  return IvLimb(a.v | b.v, 0, iv_bits_mask(a.hi > b.hi ? a.hi : b.hi));
}
inline IvLimb operator^(const IvLimb& a, const IvLimb& b) {
  a.read("^"), b.read("^");
  return IvLimb(a.v ^ b.v, 0, iv_bits_mask(a.hi > b.hi ? a.hi : b.hi));
}
inline IvLimb operator^(const IvLimb& a, uint32_t m) {
  // a lane's sign mask (u_sub_signed): x ^ 0 is x, x ^ ~0 is the complement -x - 1 as an integer (judged where it is read, like a difference)
  if (m == 0) return a;
  if (m == 0xffffffffu) return IvLimb(~a.v, -a.hi - 1, -a.lo - 1);
  return a ^ IvLimb(m);
}
inline IvLimb& IvLimb::operator|=(const IvLimb& b) { return *this = *this | b; }
inline IvLimb operator*(const IvLimb& a, const IvLimb& b) {  // the low word of a product: the Montgomery factor, masked by its caller
  if (!a.wide) a.read("*");
  IvLimb r(a.v * b.v, 0, 0xffffffffll);
  r.wide = true;
  return r;
}
inline bool operator==(const IvLimb& a, const IvLimb& b) { return a.v == b.v; }
inline bool operator!=(const IvLimb& a, const IvLimb& b) { return a.v != b.v; }

struct IvAcc {
  uint64_t v;
  unsigned __int128 lo, hi;
  IvAcc(uint64_t c = 0) : v(c), lo(c), hi(c) {}
  explicit IvAcc(const IvLimb& a) : v(a.read("a column term").v), lo(a.lo < 0 ? 0 : (uint64_t)a.lo), hi(a.hi < 0 ? 0 : (uint64_t)a.hi) {}
  void check() const {
    if (hi >> 64) u_violations().add("column sum can exceed 2^64: 2^64 * " + std::to_string((double)hi / 18446744073709551616.0));
  }
  IvAcc& operator+=(const IvAcc& b) {
    v += b.v, lo += b.lo, hi += b.hi;
    check();
    return *this;
  }
  IvAcc& operator>>=(int k) {
    v >>= k, lo >>= k, hi >>= k;
    return *this;
  }
};
inline IvAcc operator*(const IvAcc& a, const IvLimb& b) {
  b.read("a column term");
  IvAcc r;
  r.v = a.v * b.v, r.lo = a.lo * (b.lo < 0 ? 0 : (uint64_t)b.lo), r.hi = a.hi * (b.hi < 0 ? 0 : (uint64_t)b.hi);
  r.check();
  return r;
}
inline IvLimb::IvLimb(const IvAcc& a) : v((uint32_t)a.v), lo(0), hi(0xffffffffll), wide(true) {
  if (!(a.hi >> 32)) lo = (int64_t)a.lo, hi = (int64_t)a.hi, wide = false;
}

using ulimb_t = IvLimb;
using uacc_t = IvAcc;
struct UValueBound {
  double vb = INFINITY;  // value < vb * p.  UNKNOWN (infinity) until a hook of the producing function states a bound: an element made by a
                         // function without a result hook fails the next precondition that reads its value, instead of passing as "< 0 p"
};

template <class PR>
struct FpU;
template <class PR>
struct UParams;

struct UChk {
  static constexpr double EPS = 1e-9;  // the products of a few small decimals: rounding is nowhere near a bound that decides anything
  template <class PR>
  static double p_top() { return (double)UParams<PR>::P(8) + 1.0; }                       // p / 2^232 < p_top
  template <class PR>
  static double shrink() { return p_top<PR>() / 536870912.0; }                            // c = p / 2^261 < p_top / 2^29
  template <class PR>
  static int64_t top_of(double vb) { return (int64_t)(vb * p_top<PR>()); }                // value < vb p  =>  value >> 232 <= this
  template <class PR>
  static int64_t max_limb(const FpU<PR>& a, const char* who) {
    int64_t m = 0;
    for (int i = 0; i < 9; ++i) {
      if (a.l[i].lo < 0) u_violations().add(std::string(who) + ": limb " + std::to_string(i) + " of a factor can be negative (wrapped): lo = " + std::to_string(a.l[i].lo));
      if (a.l[i].hi > m) m = a.l[i].hi;
    }
    return m;
  }
  template <class PR>
  static bool n_form(const FpU<PR>& a) {
    for (int i = 0; i < 8; ++i)
      if (a.l[i].lo < 0 || a.l[i].hi >= (1 << 29)) return false;
    return a.l[8].lo >= 0 && a.l[8].hi < (int64_t(1) << 32);
  }
  static void say(const std::string& s) { u_violations().add(s); }

  template <class PR> static void zero(FpU<PR>& r) { r.vb = 0; }
  template <class PR> static void canonical(FpU<PR>& r) { r.vb = 1; }
  template <class PR> static void copy(FpU<PR>& r, const FpU<PR>& a) { r.vb = a.vb; }
  template <class PR> static void sum(FpU<PR>& r, const FpU<PR>& a, const FpU<PR>& b) { r.vb = a.vb + b.vb; }
  template <class PR> static void either(FpU<PR>& r, const FpU<PR>& a, const FpU<PR>& b) {
    for (int i = 0; i < 9; ++i) {
      r.l[i].lo = a.l[i].lo < b.l[i].lo ? a.l[i].lo : b.l[i].lo;
      r.l[i].hi = a.l[i].hi > b.l[i].hi ? a.l[i].hi : b.l[i].hi;
    }
    r.vb = a.vb > b.vb ? a.vb : b.vb;
  }
  template <int N, class PR> static void times(FpU<PR>& r, const FpU<PR>& a) { r.vb = N * a.vb; }
  template <class PR> static void mul_pre(const FpU<PR>& a, const FpU<PR>& b) {
    const double prod = (double)max_limb(a, "u_mul") * (double)max_limb(b, "u_mul");
    if (!(prod < 1.6304e18)) say("u_mul precondition: max_limb(a) * max_limb(b) = 2^58 * " + std::to_string(prod / 288230376151711744.0) + " is not below 2^60.5");   // 2^60.5 = 1.63045e18
  }
  template <class PR> static void sqr_pre(const FpU<PR>& a) {
    if (!n_form(a)) say("u_sqr precondition: the operand is not N-form (max limb " + std::to_string(max_limb(a, "u_sqr")) + ")");
  }
  template <class PR> static void mul2_pre(const FpU<PR>& a, const FpU<PR>& b, const FpU<PR>& c, const FpU<PR>& d) {
    const double s = (double)max_limb(a, "u_mul2") * (double)max_limb(b, "u_mul2") + (double)max_limb(c, "u_mul2") * (double)max_limb(d, "u_mul2");
    if (!(s <= 6.0 * 288230376151711744.0)) say("u_mul2 precondition: the two limb products sum to 2^58 * " + std::to_string(s / 288230376151711744.0) + ", above 6 * 2^58");
  }
  template <class PR> static void mont_result(FpU<PR>& r, double sum_of_products) {
    r.vb = sum_of_products * shrink<PR>() + 1.0 + EPS;
    if (r.l[8].wide) say("Montgomery result: the top limb does not fit 32 bits");
    for (int i = 0; i < 8; ++i)
      if (r.l[i].lo < 0 || r.l[i].hi >= (1 << 29)) say("Montgomery result: not N-form");
    const int64_t t = top_of<PR>(r.vb);   // N-form and 0 <= value < vb p: see the head of this file
    if ((int64_t)r.l[8].v > t) say("the model's value bound does not hold for the concrete run (Montgomery result)");
    r.l[8].lo = 0, r.l[8].hi = t, r.l[8].wide = false;
  }
  template <class PR> static void mul(FpU<PR>& r, const FpU<PR>& a, const FpU<PR>& b) { mont_result(r, a.vb * b.vb); }
  template <class PR> static void mul(FpU<PR>& r, const FpU<PR>& a, const FpU<PR>& b, const FpU<PR>& c, const FpU<PR>& d) { mont_result(r, a.vb * b.vb + c.vb * d.vb); }
  template <class PR, class... R> static void muln_pre(const FpU<PR>& a, const R&... rest) {
    if (!n_form(a)) say("u_mul3 / u_mul4 precondition: an operand is not N-form (max limb " + std::to_string(max_limb(a, "u_mul3 / u_mul4")) + ")");
    if constexpr (sizeof...(R) > 0) muln_pre(rest...);
  }
  template <class PR> static void muln(FpU<PR>& r, const FpU<PR>& a, const FpU<PR>& b, const FpU<PR>& c, const FpU<PR>& d, const FpU<PR>& e, const FpU<PR>& f) {
    mont_result(r, a.vb * b.vb + c.vb * d.vb + e.vb * f.vb);
  }
  template <class PR> static void muln(FpU<PR>& r, const FpU<PR>& a, const FpU<PR>& b, const FpU<PR>& c, const FpU<PR>& d, const FpU<PR>& e, const FpU<PR>& f,
                                      const FpU<PR>& g, const FpU<PR>& h) {
    mont_result(r, a.vb * b.vb + c.vb * d.vb + e.vb * f.vb + g.vb * h.vb);
  }
  // u_mul_shoup, exactly as stated at the function: w canonical in N-form, wq N-form with top limb < 2^29, limbs of a < 2^31, value(a) < 160 p
  template <class PR> static void shoup_pre(const FpU<PR>& a, const FpU<PR>& w, const FpU<PR>& wq) {
    if (!n_form(w) || !(w.vb <= 1 + EPS)) say("u_mul_shoup precondition: w is not a canonical N-form constant (value < " + std::to_string(w.vb) + " p)");
    for (int i = 0; i < 9; ++i)
      if (wq.l[i].lo < 0 || wq.l[i].hi >= (1 << 29)) { say("u_mul_shoup precondition: wq is not N-form with a top limb below 2^29"); break; }
    for (int i = 0; i < 9; ++i)
      if (a.l[i].lo < 0 || a.l[i].hi >= (int64_t(1) << 31)) {
        say("u_mul_shoup precondition: limb " + std::to_string(i) + " of a lies in [" + std::to_string(a.l[i].lo) + ", " + std::to_string(a.l[i].hi) + "], not in [0, 2^31)");
        break;
      }
    if (!(a.vb <= 160 + EPS)) say("u_mul_shoup precondition: value(a) < " + std::to_string(a.vb) + " p is not within 160 p");
  }
  template <class PR> static void shoup(FpU<PR>& r, const FpU<PR>&) {
    r.vb = 2;
    for (int i = 0; i < 8; ++i)
      if (r.l[i].lo < 0 || r.l[i].hi >= (1 << 29)) say("Shoup result: not N-form");
    const int64_t t = top_of<PR>(2);      // N-form and 0 <= value < 2p: limb 8 = value >> 232
    if ((int64_t)r.l[8].v > t) say("the model's value bound does not hold for the concrete run (Shoup result)");
    r.l[8].lo = 0, r.l[8].hi = t, r.l[8].wide = false;
  }
  // the memory format holds canonical elements (include/mi355zk.h): the re-packed value is < p
  template <class PR> static void from_std(FpU<PR>& r) { r.vb = 1; }
  template <int K, int S, class PR> static void sub_pre(const FpU<PR>& a, const FpU<PR>& b) {
    for (int i = 0; i < 8; ++i) {
      if (b.l[i].lo < 0 || b.l[i].hi >= (int64_t)S << 29) say("u_sub<" + std::to_string(K) + ", " + std::to_string(S) + "> precondition: limb " + std::to_string(i) + " of b reaches " + std::to_string(b.l[i].hi) + ", not below S * 2^29");
      if (a.l[i].lo < 0 || a.l[i].hi >= (int64_t(1) << 32) - ((int64_t)(S + 1) << 29) - 16) say("u_sub<" + std::to_string(K) + ", " + std::to_string(S) + "> precondition: limb " + std::to_string(i) + " of a reaches " + std::to_string(a.l[i].hi));
    }
    if (!(b.vb <= K + EPS)) say("u_sub<" + std::to_string(K) + ", " + std::to_string(S) + "> precondition: value(b) < " + std::to_string(b.vb) + " p is not within K p");
  }
  template <int K, class PR> static void sub_signed_pre(const FpU<PR>& a, const FpU<PR>& b) {
    if (!n_form(a) || !n_form(b)) say("u_sub_signed<" + std::to_string(K) + "> precondition: an operand is not N-form");
    if (!(a.vb + b.vb <= K + EPS)) say("u_sub_signed<" + std::to_string(K) + "> precondition: value(a) + value(b) < " + std::to_string(a.vb + b.vb) + " p is not within K p");
  }
  template <int K, class PR> static void sub_lazy(FpU<PR>& t, const FpU<PR>& a) {
    t.vb = a.vb + K;
    for (int i = 0; i < 8; ++i)
      if (!t.l[i].fits()) say("u_sub: limb " + std::to_string(i) + " of the difference can wrap: [" + std::to_string(t.l[i].lo) + ", " + std::to_string(t.l[i].hi) + "]");
  }
  template <class PR> static void carried_nonneg(FpU<PR>& r) {
    const int64_t t = top_of<PR>(r.vb);   // N-form, 0 <= value < vb p: see the head of this file
    if ((int64_t)r.l[8].v > t) say("the model's value bound does not hold for the concrete run (carried difference)");
    r.l[8].lo = 0, r.l[8].hi = t;
  }
  template <int K, class PR> static void require_lt(const FpU<PR>& a) {
    if (!n_form(a)) say("u_to_std_lt" + std::to_string(K) + "p precondition: not N-form");
    if (!(a.vb <= K + EPS)) say("u_to_std_lt" + std::to_string(K) + "p precondition: value < " + std::to_string(a.vb) + " p");
  }
};

}  // namespace zk

#include "../../phase2-bn254_amd/csrc/curveu.hpp"
