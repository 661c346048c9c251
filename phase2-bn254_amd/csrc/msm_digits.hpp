#pragma once
// Stage 1 of the Pippenger pipeline (msm_impl.hpp has the design): the signed digits of one scalar, power-of-two or mixed-radix
// windows.  __host__ __device__: the digit kernels of msm_partition.hip run it per lane, and the host self-test hook
// (msm_partition.hip: msm_selftest_digits, tests/test_msm_digits_host.py) runs the very same functions on one scalar.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "msm_common.hpp"

namespace zk {

// ------------------------------------------------------------------------------------------------
// 1. digits.  density == nullptr: FullDensity (source.rs:80-99): base of exponent i is base_offset+i.
//    Otherwise bit i of `density` selects exponent i and the bases are compacted (source.rs:101-118):
//    rank(i) = dprefix[i/32] + popc(density[i/32] & ((1<<i%32)-1)).
// q = q div M, returns q mod M   (q on 8 words of which only words 0..top can be non-zero; M a small constant).  `top` is
// uniform over the launch (it follows from the window number), so the skipped word steps are skipped by scalar branches: the
// dividend loses ~42 bits with every pair of digits taken off, and the multiword work is what the digit extraction costs.
template <uint32_t M>
__host__ __device__ __forceinline__ uint32_t msm_divmod_small(uint32_t q[8], int top) {
  uint32_t rem = 0;
#pragma unroll
  for (int l = 7; l >= 0; --l) {
    if (l > top) continue;
    const uint64_t cur = ((uint64_t)rem << 32) | q[l];
    q[l] = (uint32_t)(cur / M);
    rem = (uint32_t)(cur % M);
  }
  return rem;
}

// two mixed-radix digits at once: (r0 + B r1) = q mod B^2, q = q div B^2, B = M * 2^sh (sh <= 22).  One multiword division by
// M^2 instead of two by M.
template <uint32_t M>
__host__ __device__ __forceinline__ void msm_two_digits(uint32_t q[8], uint32_t sh, uint32_t& r0, uint32_t& r1, int top) {
  const uint64_t low = (((uint64_t)q[1] << 32) | q[0]) & ((1ull << (2 * sh)) - 1ull);
#pragma unroll
  for (int rep = 0; rep < 2; ++rep) {
#pragma unroll
    for (int l = 0; l < 8; ++l)
      if (l <= top) q[l] = (q[l] >> sh) | (l < 7 ? q[l + 1] << (32 - sh) : 0u);
  }
  const uint32_t rem = msm_divmod_small<M * M>(q, top);
  const uint64_t pv = low + ((uint64_t)rem << (2 * sh));  // < B^2 < 2^52
  const uint64_t hi = (pv >> sh) / M;                      // pv div B
  r1 = (uint32_t)hi;
  r0 = (uint32_t)(pv - hi * ((uint64_t)M << sh));
}

// q = q div M^k (M a small odd constant, k uniform over the launch), in steps of M^4 and M (two instantiations per multiplier: the
// digit kernels carry seven multipliers and must stay inside the instruction cache); nbits: q < 2^nbits.
template <uint32_t M>
__host__ __device__ __forceinline__ void msm_div_pow(uint32_t q[8], uint32_t k, int& nbits, int flog_m) {
  constexpr uint32_t M4 = M * M * M * M;
#pragma unroll 1
  for (; k >= 4; k -= 4) {
    (void)msm_divmod_small<M4>(q, nbits > 0 ? (nbits - 1) >> 5 : 0);
    nbits -= 4 * flog_m;
  }
#pragma unroll 1
  for (; k >= 1; k -= 1) {
    (void)msm_divmod_small<M>(q, nbits > 0 ? (nbits - 1) >> 5 : 0);
    nbits -= flog_m;
  }
}

// Digits of one scalar (canonical limbs s[0..7], s[8] = 0) from window w_first on: emit(w, d, neg) for w_first <= w < w_stop,
// d = |digit| (0 = no bucket), neg = SIGN_BIT for a negative digit.  The carry chain of the signed digits starts at w_first
// with carry 0: exact for w_first == 0; for w_first > 0 the carry OUT of window w_first is exact unless that window's raw digit
// sits on the boundary (then it depends on the carry in, which was not computed): the function returns false BEFORE emitting
// anything, and the caller starts again from window 0.  (The digit of window w_first itself may be off by the missing carry:
// callers that start above 0 do not use it.)
// RM: the geometry's multiplier G.rmul as a compile-time constant (1 = power-of-two windows): every digit kernel is instantiated
// per multiplier, so that it carries ONE set of constant divisions instead of seven behind a switch (instruction cache).
template <uint32_t RM, class Emit>
__host__ __device__ __forceinline__ bool msm_scalar_digits_from(const uint32_t s[9], const MsmGeom& G, uint32_t w_first, uint32_t w_stop, Emit emit) {
  uint32_t carry = 0;
  if constexpr (RM != 1) {
    // mixed radix: repeatedly  low = q mod 2^rshift;  q >>= rshift;  (q, r) = divmod(q, rmul);  digit = low + 2^rshift * r
    uint32_t q[8];
    const uint32_t sh = G.rshift, B = RM << sh;
    constexpr int flog_m = RM >= 8 ? 3 : RM >= 4 ? 2 : 1;  // floor(log2 rmul): a digit takes at least sh + flog_m bits off q
    int nbits = 254;                                           // q < 2^nbits (exponents are < r < 2^254)
    if (w_first == 0) {
#pragma unroll
      for (int l = 0; l < 8; ++l) q[l] = s[l];
    } else {
      // q = s div B^w_first = (s >> (sh * w_first)) div rmul^w_first: one multiword shift and one or two multiword divisions
      // instead of w_first digit steps (uniform over the launch: scalar branches, static register indices)
      const uint32_t bits = sh * w_first, ls = bits >> 5, bs = bits & 31;
#pragma unroll
      for (int l = 0; l < 8; ++l) {
        uint32_t lo = 0, hi = 0;
#pragma unroll
        for (int c = 0; c < 8; ++c)
          if (ls == (uint32_t)c) {
            lo = l + c < 8 ? s[l + c < 8 ? l + c : 0] : 0u;
            hi = l + c + 1 < 8 ? s[l + c + 1 < 8 ? l + c + 1 : 0] : 0u;
          }
        q[l] = bs ? (lo >> bs) | (hi << (32 - bs)) : lo;
      }
      nbits -= (int)bits;
      msm_div_pow<RM>(q, w_first, nbits, flog_m);
    }
    uint32_t pending = 0;
    bool have_pending = false;
    for (uint32_t w = w_first; w < w_stop; ++w) {
      const int top = nbits > 0 ? (nbits - 1) >> 5 : 0;
      uint32_t d, neg = 0;
      if (w + 1 < G.W) {
        uint32_t raw;
        if (have_pending) {
          raw = pending;
          have_pending = false;
        } else if (w + 2 < G.W) {  // this window and the next one, neither of them the top window
          msm_two_digits<RM>(q, sh, raw, pending, top);  // division by compile-time constants (multiply-high)
          have_pending = true;
          nbits -= 2 * (int)(sh + flog_m);
        } else {
          const uint32_t low = q[0] & ((1u << sh) - 1u);
#pragma unroll
          for (int l = 0; l < 8; ++l) q[l] = (q[l] >> sh) | (l < 7 ? q[l + 1] << (32 - sh) : 0u);
          nbits -= (int)(sh + flog_m);
          const uint32_t rem = msm_divmod_small<RM>(q, top);
          raw = low + (rem << sh);
        }
        if (w == w_first && w_first != 0 && raw == G.nb) return false;  // carry out = carry in: not known here
        d = raw + carry;
        carry = 0;
        if (d > G.nb) {          // d in (B/2, B]  ->  d - B in (-B/2, 0]
          d = B - d;
          neg = d ? SIGN_BIT : 0;
          carry = 1;
        }
      } else {
        d = q[0] + carry;        // top digit, unsigned: <= nb by the choice of B (make_geom_radix)
      }
      emit(w, d, neg);
    }
    return true;
  } else {
  for (uint32_t w = w_first; w < w_stop; ++w) {
    const uint32_t width = G.width[w], bit = G.shift[w];
    const uint32_t limb = bit >> 5, off = bit & 31;
    // (static indices under a uniform condition: a dynamic s[limb] would move the whole array, in every path of the
    // kernel, from registers to scratch memory)
    uint32_t lo = 0, hi = 0;
#pragma unroll
    for (int l = 0; l < 8; ++l)
      if (limb == (uint32_t)l) { lo = s[l]; hi = s[l + 1]; }
    const uint64_t two = (uint64_t)lo | ((uint64_t)hi << 32);
    const uint32_t raw = (uint32_t)(two >> off) & ((1u << width) - 1u);
    if (w == w_first && w_first != 0 && w + 1 < G.W && raw == (1u << (width - 1))) return false;  // carry out = carry in
    uint32_t d = raw + carry;
    uint32_t neg = 0;
    carry = 0;
    if (w + 1 < G.W && d > (1u << (width - 1))) {  // d in (2^(width-1), 2^width]  ->  d - 2^width in (-2^(width-1), 0]
      d = (1u << width) - d;
      neg = (d != 0) ? SIGN_BIT : 0;
      carry = 1;
    }
    emit(w, d, neg);
  }
  return true;
  }
}

// The digits of windows w_start <= w < w_stop (a multi-GPU rank that owns a group of windows; the whole range on one GPU): the
// chain starts ONE window below w_start -- the carry into w_start is all the lower windows contribute -- and only the rare
// scalar whose digit there sits exactly on the sign boundary (one in B) walks the chain from window 0.
template <uint32_t RM, class Emit>
__host__ __device__ __forceinline__ void msm_scalar_digits(const uint32_t s[9], const MsmGeom& G, uint32_t w_start, uint32_t w_stop, Emit emit) {
  if (w_start == 0) {  // the whole range (one GPU): its own copy of the chain, specialised for a start at window 0
    (void)msm_scalar_digits_from<RM>(s, G, 0, w_stop, emit);
    return;
  }
  const uint32_t w_first = w_start >= 2 ? w_start - 1 : 0;
  auto windowed = [&](uint32_t w, uint32_t d, uint32_t neg) {
    if (w >= w_start) emit(w, d, neg);
  };
  // (one inlined copy of the chain for every start above 0: the second trip only runs for the boundary scalars)
  uint32_t from = w_first;
#pragma unroll 1
  for (int attempt = 0; attempt < 2; ++attempt) {
    if (msm_scalar_digits_from<RM>(s, G, from, w_stop, windowed)) return;
    from = 0;
  }
}

// run `stmt` with RM bound to G.rmul as a compile-time constant
#define ZK_DISPATCH_RMUL(rmul, stmt)                      \
  switch (rmul) {                                          \
    case 1: { constexpr uint32_t RM = 1; stmt; } break;    \
    case 3: { constexpr uint32_t RM = 3; stmt; } break;    \
    case 5: { constexpr uint32_t RM = 5; stmt; } break;    \
    case 7: { constexpr uint32_t RM = 7; stmt; } break;    \
    case 9: { constexpr uint32_t RM = 9; stmt; } break;    \
    case 11: { constexpr uint32_t RM = 11; stmt; } break;  \
    case 13: { constexpr uint32_t RM = 13; stmt; } break;  \
    default: { constexpr uint32_t RM = 15; stmt; } break;  \
  }

}  // namespace zk
