// Windowed scalar multiplication k * P on the U-form Jacobian arithmetic of curveu.hpp, stated ONCE for G1 and G2, device and host:
// the point FFT's butterflies (point_fft_impl.hpp), the G2 batch_exp (scalar_mul.hip: batch_exp_win_u2_kernel) and the host self-test
// of that kernel (field_ops.hip) all run this program.
//
// Each lane keeps a table of 1P..8P (Jacobian + Z^2 + Z^3) laid out [entry][lane] and walks fixed signed 4-bit windows over it, so
// the 64 lanes of a wave add at the same places although their scalars differ.  Table build and windows run through ONE loop of
// steps (load entry, double?, add entry, store entry) around a single inlined doubling and a single inlined table addition: the Fq2
// group law is > 100 KB of gfx950 code per copy, and out-of-line calls with these operands go through scratch and crawl.
//   steps 0..6                 table:  2P = 2*1P, 3P = 2P + 1P, 4P = 2*2P, 5P = 4P + 1P, 6P = 2*3P, 7P = 6P + 1P, 8P = 2*4P
//   steps 7..7+PER*WINDOWS-1   WINDOWS windows, top digit first, of PER steps: four doublings (the fourth adds the window's digit
//                              entry) and, SPLIT, the digit of the second half through the endomorphism
// SPLIT: k = k1 + k2 lambda with both halves < 2^128 (glv.hpp), half the doublings; exact only where the endomorphism IS lambda.
#pragma once

#include "curveu.hpp"
#include "device_util.hpp"
#include "glv.hpp"

namespace zk {

// ---- the two groups: types, group law, endomorphism and split, under one set of names
struct G1U {
  using Acc = JacU<FqParams>;       // accumulator
  using Tab = JacTabU<FqParams>;    // table entry
  using Aff = G1Affine;             // affine raw record
  using Z = Fq;                     // the field of a Z coordinate
  static constexpr bool ENDO_EVERYWHERE = true;           // phi = lambda on all of E(Fq), a group of prime order: no plain form needed
  static constexpr uint64_t PFFT_LANES = 1ull << 20;      // point FFT: lanes per launch (the table is 8 x 192 B per lane)
  ZK_HD static Acc dbl(const Acc& a) { return jacu_double(a); }
  ZK_HD static void add_tab(Acc& a, const Tab& e, bool negate) { jacu_add_tab(a, e, negate); }
  ZK_HD static Tab tab_entry(const Acc& a) { return jacu_tab_entry(a); }
  ZK_HD static Acc from_affine(const Aff& p) {            // not infinity
    const FqU c266 = UPow2<FqParams, 266>::get();         // x*2^256 * 2^266 / 2^261 = x * 2^261
    return Acc{u_mul(u_from_std(p.x), c266), u_mul(u_from_std(p.y), c266), UPow2<FqParams, 261>::get()};
  }
  ZK_HD static Jacobian<Z> to_std(const Acc& a) { return jacu_to_std(a); }
  ZK_HD static bool is_order_two_zero(const FqU& z) { return u_is_zero_lt2p(z); }
  struct Endo {
    FqU betaU;                                            // beta, 2^261 domain
    ZK_HD static Endo prepare() { return Endo{u_mul(u_from_std(glv_beta()), UPow2<FqParams, 266>::get())}; }
    ZK_HD Tab apply(Tab e) const {                        // phi(X, Y, Z) = (beta X, Y, Z)
      e.x = u_mul(e.x, betaU);                            // X < 6p: < 1.08p
      return e;
    }
  };
  ZK_HD static GlvSplit split(const uint32_t k[8]) { return glv_split(k); }
};

struct G2U {
  using Acc = JacU2;
  using Tab = JacTabU2;
  using Aff = G2Affine;
  using Z = Fq2;
  static constexpr bool ENDO_EVERYWHERE = false;          // psi = mu in the order-r subgroup ONLY: the plain form is the default
  static constexpr uint64_t PFFT_LANES = 1ull << 19;      // (8 x 368 B per lane)
  ZK_HD static Acc dbl(const Acc& a) { return jacu2_double(a); }
  ZK_HD static void add_tab(Acc& a, const Tab& e, bool negate) { jacu2_add_tab(a, e, negate); }
  ZK_HD static Tab tab_entry(const Acc& a) { return jacu2_tab_entry(a); }
  ZK_HD static Acc from_affine(const Aff& p) {
    const Tab e = jacu2_tab_from_affine(p.x, p.y);        // (x, y, one) in the 2^261 domain
    return Acc{e.x, e.y, e.z};
  }
  ZK_HD static Jacobian<Z> to_std(const Acc& a) { return jacu2_to_std(a); }
  ZK_HD static bool is_order_two_zero(const Fq2U& z) { return u_is_zero_lt2p(z.c0) && u_is_zero_lt2p(z.c1); }
  struct Endo {
    Fq2U cxU, cyU;                                        // the constants of psi, 2^261 domain, < 2p
    ZK_HD static Endo prepare() {
      const FqU c266 = UPow2<FqParams, 266>::get();
      const Fq2 cx = glv2_cx(), cy = glv2_cy();
      return Endo{Fq2U{u_mul(u_from_std(cx.c0), c266), u_mul(u_from_std(cx.c1), c266)},
                  Fq2U{u_mul(u_from_std(cy.c0), c266), u_mul(u_from_std(cy.c1), c266)}};
    }
    ZK_HD Tab apply(const Tab& e) const { return jacu2_tab_psi(e, cxU, cyU); }
  };
  ZK_HD static GlvSplit split(const uint32_t k[8]) {      // both halves non-negative
    const Glv2Split s = glv2_split(k);
    GlvSplit g;
#pragma unroll
    for (int i = 0; i < 5; ++i) { g.k1[i] = s.k1[i]; g.k2[i] = s.k2[i]; }
    g.neg1 = g.neg2 = false;
    return g;
  }
};

// one step of the program: entries are 1..8, 0 = none
struct WinStep {
  uint32_t load = 0, dbl = 0, add = 0, store = 0;
  bool clear = false, negate = false, endo = false;       // clear: the accumulator restarts at infinity (first window step)
};

// digit j of a signed_nibbles string: the magnitude, and through `negative` its sign.  The word is picked by a chain of selects over
// constant indices, whatever the arrays are part of.
template <int N>
ZK_HD uint32_t win_word(const uint32_t (&a)[N], int w) {
  uint32_t r = 0;
#pragma unroll
  for (int i = 0; i < N; ++i) r = i == w ? a[i] : r;
  return r;
}
template <int NW, int NS>
ZK_HD uint32_t win_digit(const uint32_t (&mag)[NW], const uint32_t (&sgn)[NS], int j, bool& negative) {
  negative = ((win_word(sgn, j >> 5) >> (j & 31)) & 1u) != 0;
  return (win_word(mag, j >> 3) >> (4 * (j & 7))) & 15u;
}

// The program over the digits of one scalar.  WINDOWS is the caller's: 33 (SPLIT) / 64 for canonical scalars (< r: the halves are
// < 2^128 and a plain scalar's nibble 63 carries nothing out), 40 / 65 for any 256 bits (every nibble of the five words of a half; the
// 64 nibbles and the carry out of the last).  Doubling infinity returns at once, so leading zero windows cost nothing.
// The digit state is the CALLER's local arrays (`Digits` names their shapes): as members of one object they cost the G1 stage kernel
// 33 VGPRs and a wave per SIMD (hipcc 7, measured).
template <class G, bool SPLIT, int WINDOWS>
struct WindowMul {
  using Acc = typename G::Acc;
  using Tab = typename G::Tab;
  static constexpr int TABLE_STEPS = 7, PER = SPLIT ? 5 : 4, STEPS = TABLE_STEPS + PER * WINDOWS;
  static constexpr int NW = (WINDOWS + 7) / 8, NS = (NW + 3) / 4;
  using Mag = uint32_t[NW];   // |d_j|, a nibble each, of the signed digits d_j in [-8, 8]: m = sum d_j 16^j
  using Sgn = uint32_t[NS];   // bit j = (d_j < 0)

  // the digits of k (SPLIT: of both halves, with the halves' signs and the endomorphism's constants; plain: mag2, sgn2, endo stay unset)
  ZK_HD static void digits(const uint32_t k[8], Mag& mag1, Sgn& sgn1, Mag& mag2, Sgn& sgn2, bool& neg1, bool& neg2, typename G::Endo& endo) {
    neg1 = neg2 = false;
    if constexpr (SPLIT) {
      const GlvSplit g = G::split(k);
      signed_nibbles<NW, 5>(g.k1, mag1, sgn1);
      signed_nibbles<NW, 5>(g.k2, mag2, sgn2);
      neg1 = g.neg1;
      neg2 = g.neg2;
      endo = G::Endo::prepare();
    } else {
      signed_nibbles<NW, 8>(k, mag1, sgn1);
    }
  }

  ZK_HD static WinStep decode(int step, const Mag& mag1, const Sgn& sgn1, const Mag& mag2, const Sgn& sgn2, bool neg1, bool neg2) {
    WinStep s;
    if (step < TABLE_STEPS) {
      constexpr uint32_t PROG[TABLE_STEPS] = {0x1102, 0x0013, 0x2104, 0x0015, 0x3106, 0x0017, 0x4108};  // nibbles: load, double, add, store
      const uint32_t pr = PROG[step];
      s.load = pr >> 12;
      s.dbl = (pr >> 8) & 15u;
      s.add = (pr >> 4) & 15u;
      s.store = pr & 15u;
    } else {
      const int m = step - TABLE_STEPS;
      s.clear = m == 0;
      const int win = m / PER, sub = m - PER * win, j = WINDOWS - 1 - win;
      bool negative = false;
      if (sub < 4) {
        s.dbl = 1;
        if (sub == 3) {
          s.add = win_digit(mag1, sgn1, j, negative);
          s.negate = negative != neg1;
        }
      } else {
        s.add = win_digit(mag2, sgn2, j, negative);
        s.negate = negative != neg2;
        s.endo = true;
      }
    }
    return s;
  }

  // acc after step s over the lane's table (tab: the lane's entry 1; entry e at tab[(e - 1) * stride]).  CANON: curves with points of
  // order two (records on no curve, whose multiples live on y^2 = x^3 + (y0^2 - x0^3)): a result with 2 Y Z == 0 is made the literal
  // infinity.  An infinite entry (d P for a small d: off the curve only) is skipped, which is what adding infinity means; the test reads
  // the entry AFTER the endomorphism, and psi of an infinite entry is not the literal infinity -- the split forms never meet one.
  template <bool CANON>
  ZK_HD static Acc exec(Acc acc, const WinStep& s, Tab* tab, uint64_t stride, const typename G::Endo& endo) {
    if (s.clear) acc = Acc::zero();
    if (s.load) {
      const Tab e = copy16_load(tab + (uint64_t)(s.load - 1) * stride);
      acc = Acc{e.x, e.y, e.z};
    }
    if (s.dbl) {
      acc = G::dbl(acc);
      if constexpr (CANON)
        if (G::is_order_two_zero(acc.z)) acc = Acc::zero();
    }
    if (s.add) {
      Tab e = copy16_load(tab + (uint64_t)(s.add - 1) * stride);
      if constexpr (SPLIT)
        if (s.endo) e = endo.apply(e);
      if (!e.z.limbs_all_zero()) {
        G::add_tab(acc, e, s.negate);
        if constexpr (CANON)
          if (G::is_order_two_zero(acc.z)) acc = Acc::zero();   // (the addition doubles when acc == e)
      }
    }
    if (s.store) copy16_store(tab + (uint64_t)(s.store - 1) * stride, G::tab_entry(acc));
    return acc;
  }
};

}  // namespace zk
