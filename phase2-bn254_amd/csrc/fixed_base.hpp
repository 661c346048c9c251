// Fixed-base scalar multiplication k * P over a window table of ONE base, stated once for G1 and G2, device and host: the kernels of
// fixed_base.hip, the host self-test hook and the tests all run this recoding and this step program.
//
// Geometry: signed FB_WIDTH-bit windows, FB_WINDOWS of them.  The table holds T[w][j - 1] = (j * 2^(FB_WIDTH w)) * P for w < FB_WINDOWS and
// j = 1 .. FB_HALF, affine raw records (4096 entries: 256 KiB for G1, 512 KiB for G2), so a scalar costs NO doubling and at most FB_WINDOWS
// mixed additions:  k = sum_w d_w 2^(8 w),  d_w in [-128, 128],  k P = sum_w sign(d_w) T[w][|d_w| - 1].
// The additions are the general routines of curveu.hpp (equal, opposite and infinite operands handled), NOT a stripped variant: for a
// canonical k over ONE base the partial sum never equals MINUS the entry being added (that would make k == 0 mod r), but it can EQUAL it --
// exactly for k = 2 * 48 * 2^248 - r, whose low windows sum to 48 * 2^248 - r == 48 * 2^248 (mod r) -- and jacu_add_mixed then doubles.
// Over several bases (fixed_base_accumulate) all of these cases are ordinary.
#pragma once

#include "window_mul.hpp"

namespace zk {

constexpr int FB_WIDTH = 8;                                  // bits per window (any other value ships with an A/B in profiles/fixed_base.md)
constexpr int FB_WINDOWS = (256 + FB_WIDTH - 1) / FB_WIDTH;  // 32
constexpr int FB_HALF = 1 << (FB_WIDTH - 1);                 // 128 entries per window: the magnitudes 1 .. 128
constexpr int FB_ENTRIES = FB_WINDOWS * FB_HALF;             // 4096
static_assert(FB_WIDTH == 8, "fixed_base_digit reads whole bytes of the scalar");

// Digit w of k given the carry out of digit w - 1 (0 for w == 0):  sum_w d_w 2^(8 w) == k as integers for every k whose last carry is 0.
// byte + carry in [0, 256]:  > 128 becomes byte + carry - 256 (in [-127, 0]) and carries one.  A canonical k < r has k >> 248 <= 0x30, so
// its top digit is <= 49 and nothing leaves window 31; any other 256-bit k loses that carry (its record is unspecified, never out of range).
ZK_HD int fixed_base_digit(const uint32_t (&k)[8], int w, uint32_t& carry) {
  const uint32_t v = ((win_word(k, w >> 2) >> (8 * (w & 3))) & 255u) + carry;
  carry = v > (uint32_t)FB_HALF ? 1u : 0u;
  return (int)v - (carry ? 2 * FB_HALF : 0);
}

// table index of the entry |d| 2^(8 w) P, d != 0; the magnitude is clamped so that no digit, whatever the scalar, leaves the table
ZK_HD uint32_t fixed_base_index(int w, int d) {
  uint32_t mag = (uint32_t)(d < 0 ? -d : d);
  mag = mag > (uint32_t)FB_HALF ? (uint32_t)FB_HALF : mag;
  return (uint32_t)w * FB_HALF + (mag - 1u);
}

// acc += (+/-) e for an affine table entry (memory format); an all-zero entry is the identity and adds nothing
ZK_HD void fixed_base_add(JacU<FqParams>& acc, const G1Affine& e, bool negate) {
  if (e.is_zero()) return;
  const FqU c266 = UPow2<FqParams, 266>::get();             // x*2^256 * 2^266 / 2^261 = x * 2^261
  jacu_add_mixed(acc, u_mul(u_from_std(e.x), c266), u_mul(u_from_std(e.y), c266), negate);
}
ZK_HD void fixed_base_add(JacU2& acc, const G2Affine& e, bool negate) {
  if (e.is_zero()) return;
  const FqU c266 = UPow2<FqParams, 266>::get(), one = UPow2<FqParams, 261>::get();
  JacTabU2 t;                                               // the entry with Z = Z^2 = Z^3 = one: jacu2_add_tab is the mixed addition
  t.x = Fq2U{u_mul(u_from_std(e.x.c0), c266), u_mul(u_from_std(e.x.c1), c266)};   // < 2p
  t.y = Fq2U{u_mul(u_from_std(e.y.c0), c266), u_mul(u_from_std(e.y.c1), c266)};
  t.z = t.zz = t.zzz = Fq2U{one, FqU::zero()};
  t.pad[0] = t.pad[1] = 0;
  jacu2_add_tab(acc, t, negate);
}

// acc += k * P: FB_WINDOWS steps of "digit, load entry, add", zero digits skipped.  load(index) returns the affine entry at a table index.
// The accumulator is the caller's, so a sum over SEVERAL bases (fixed_bases_lincomb_kernel, one table per base) runs this once per base into
// one accumulator.  There the partial sum is whatever the earlier bases left: it can equal the entry, be its negative (the sum passes through
// the identity) or be the identity in the middle of a row, and the general additions above take all three.
template <class G, class Load>
ZK_HD void fixed_base_accumulate(typename G::Acc& acc, const uint32_t (&k)[8], Load&& load) {
  uint32_t carry = 0;
#pragma unroll 1
  for (int w = 0; w < FB_WINDOWS; ++w) {
    const int d = fixed_base_digit(k, w, carry);
    if (d != 0) fixed_base_add(acc, load(fixed_base_index(w, d)), d < 0);
  }
}

// k * P: the same from the identity
template <class G, class Load>
ZK_HD typename G::Acc fixed_base_run(const uint32_t (&k)[8], Load&& load) {
  typename G::Acc acc = G::Acc::zero();
  fixed_base_accumulate<G>(acc, k, load);
  return acc;
}

}  // namespace zk
