// Bound checker for the G1 bucket arithmetic: the functions of csrc/fieldu.hpp and csrc/curveu.hpp that a G1 addition runs, INSTANTIATED on
// limbs that carry worst-case intervals (tests/cpp/u_interval.hpp -- read its head for what is tracked and how limb 8 is judged).  Host
// compiler only; tests/test_u_bounds_host.py builds and runs it.
//   test_u_bounds_host            every formula below with operands anywhere inside the stated invariants; prints what it found;
//                                 exit 0 if nothing can overflow and every stated precondition is met, 1 otherwise
//   test_u_bounds_host bite       the y3 product of the mixed addition with x3, d and ny1 ALL left un-carried: u_mul2's column bound is
//                                 broken and the checker must say so; exit 0 if it does, 1 if it stays silent
//   test_u_bounds_host bite_sqr   u_sqr of an operand with limbs up to 3 * 2^29: a 64-bit column sum passes 2^64 and the column intervals
//                                 themselves must report it; exit 0 if they do
// The operands are the invariants themselves, not reachable points: X < 6p, Y, ZZ, ZZZ < 2p, N-form (limbs 0..7 anywhere in
// [0, 2^29), limb 8 anywhere in [0, value bound >> 232]); loaded coordinates < p.  The concrete values that ride along only steer the
// branches (main path: ZZ3 != 0).
#include <cstring>

#include "u_interval.hpp"

using namespace zk;
using P = FqParams;
using F = FpU<P>;
using A = XYZZU<P>;

static uint32_t rng_state = 12345;
static uint32_t rnd() {
  rng_state = rng_state * 1664525u + 1013904223u;
  return rng_state >> 3;
}

// an N-form element with value < vb p: limbs 0..7 anywhere in [0, 2^29), limb 8 anywhere in [0, (vb p) >> 232]; a concrete value < p rides along
static F any_below(double vb) {
  F r;
  for (int i = 0; i < 8; ++i) r.l[i] = IvLimb(rnd() & U_MASK, 0, U_MASK);
  r.l[8] = IvLimb(rnd() % UParams<P>::P(8), 0, UChk::top_of<P>(vb));
  r.vb = vb;
  return r;
}
static A any_acc() { return A{any_below(6), any_below(2), any_below(2), any_below(2)}; }

static void expect(const F& a, double vb, const char* what) {
  if (!UChk::n_form(a)) u_violations().add(std::string("result ") + what + " is not N-form");
  if (!(a.vb <= vb)) u_violations().add(std::string("result ") + what + " < " + std::to_string(a.vb) + " p breaks the invariant < " + std::to_string(vb) + " p");
}
static void expect_acc(const A& a) {
  expect(a.x, 6, "X"), expect(a.y, 2, "Y"), expect(a.zz, 2, "ZZ"), expect(a.zzz, 2, "ZZZ");
  std::printf("  %-44s X < %.3f p  Y < %.3f p  ZZ < %.3f p  ZZZ < %.3f p\n", u_violations().where, a.x.vb, a.y.vb, a.zz.vb, a.zzz.vb);
}

static int run_all() {
  for (int neg = 0; neg < 2; ++neg) {
    u_violations().where = neg ? "xyzzu_add_mixed (negated)" : "xyzzu_add_mixed";
    A acc = any_acc();
    xyzzu_add_mixed_u(acc, any_below(1), any_below(1), neg != 0);
    expect_acc(acc);
    u_violations().where = neg ? "xyzzu_add_mixed (empty accumulator, negated)" : "xyzzu_add_mixed (empty accumulator)";
    acc = A::zero();
    xyzzu_add_mixed_u(acc, any_below(1), any_below(1), neg != 0);
    expect_acc(acc);
    u_violations().where = neg ? "xyzzu_double_affine (signed y, negated)" : "xyzzu_double_affine (signed y)";
    expect_acc(xyzzu_double_affine(any_below(1), u_signed_y(any_below(1), neg != 0)));
  }
  for (int s = 0; s < 4; ++s) {
    u_violations().where = "xyzzu_from_affine_pair";
    expect_acc(xyzzu_from_affine_pair_u(any_below(1), any_below(1), (s & 1) != 0, any_below(1), any_below(1), (s & 2) != 0, false));
  }
  {
    u_violations().where = "xyzzu_from_affine_pair (the same point)";
    const F x = any_below(1), y = any_below(1);
    expect_acc(xyzzu_from_affine_pair_u(x, y, true, x, y, true, true));
  }
  {
    u_violations().where = "xyzzr_add";
    A acc = any_acc();
    xyzzr_add(acc, any_acc());
    expect_acc(acc);
    u_violations().where = "xyzzu_double";
    expect_acc(xyzzu_double(any_acc()));
  }
  {
    u_violations().where = "xyzzu_to_r";
    (void)xyzzu_to_r(any_acc());   // the conversions themselves are plain-word code: their preconditions are what is tested here
    u_violations().where = "xyzzr_store";
    (void)xyzzr_store(any_acc());
  }
  for (const auto& s : u_violations().list) std::printf("VIOLATION %s\n", s.c_str());
  std::printf("%zu violations\n", u_violations().list.size());
  return u_violations().list.empty() ? 0 : 1;
}

// The combination the issue names: x3, d and ny1 all un-carried.  x3 has limbs < 5 * 2^29, so d = q + 8p - x3 needs S = 5 and has limbs
// < 7 * 2^29; with ny1 < 2^30 a column of R*D + NY1*PPP can hold 9 * 7 + 9 * 2 + 9 = 90 products of 2^58: 2^64.5.
static int run_bite() {
  u_violations().where = "y3 with x3, d, ny1 un-carried";
  const F r = any_below(5.02), rr = any_below(1.16), q = any_below(1.06), ppp = any_below(1.1), y1 = any_below(2);
  const F t = u_add(ppp, u_dbl(q));
  const F x3 = u_sub_lazy<4, 3>(rr, t);
  const F d = u_sub_lazy<8, 5>(q, x3);
  const F ny1 = u_sub_lazy<3, 1>(F::zero(), y1);
  (void)u_mul2(r, d, ny1, ppp);
  // (whether a column's interval itself passes 2^64 depends on the limbs of 8p - 4p and of 3p for this modulus; what the checker must
  // report either way is that the call no longer meets the bound u_mul2 states, 6 * 2^58, which is what keeps EVERY column below 2^64)
  bool said = false;
  for (const auto& s : u_violations().list) {
    std::printf("REPORTED %s\n", s.c_str());
    if (s.find("column sum can exceed 2^64") != std::string::npos || s.find("u_mul2 precondition") != std::string::npos) said = true;
  }
  return said ? 0 : 1;
}

// The other half: the column intervals themselves.  u_sqr of an operand whose limbs reach 3 * 2^29 (an un-carried P or R): a column holds four
// cross products of 6 * 3 * 2^58, a square of 9 * 2^58 and the Montgomery terms -- past 2^64, and the IvAcc sums must say so (not only sqr_pre).
static int run_bite_sqr() {
  u_violations().where = "u_sqr of limbs up to 3 * 2^29";
  F a = any_below(4);
  for (int i = 0; i < 8; ++i) a.l[i] = IvLimb(a.l[i].v, 0, 3ll * (1 << 29) - 1);
  (void)u_sqr(a);
  bool column = false;
  for (const auto& s : u_violations().list) {
    std::printf("REPORTED %s\n", s.c_str());
    if (s.find("column sum can exceed 2^64") != std::string::npos) column = true;
  }
  return column ? 0 : 1;
}

int main(int argc, char** argv) {
  if (argc > 1 && !std::strcmp(argv[1], "bite")) return run_bite();
  if (argc > 1 && !std::strcmp(argv[1], "bite_sqr")) return run_bite_sqr();
  return run_all();
}
