#pragma once
// Pippenger multi-scalar multiplication over BN254 G1 / G2 for gfx950 (MI355X).
//
// Replaces, behind the C ABI of include/mi355zk.h, the reference's
//   bellman/src/multiexp.rs:330-355  multiexp()          (window choice, density contract)
//   bellman/src/multiexp.rs:53-157   multiexp_inner()    (bucket fill, summation by parts, window join)
//   bellman/src/source.rs:36-70      (Arc<Vec<G>>, usize) Source: cursor + error semantics
// and the group law underneath (pairing/src/bn256/ec.rs:301-536).
//
// MI355X design (DESIGN.md "MSM"), not the reference's one-thread-per-window scan:
//   1. msm_digits_plain_kernel  every scalar -> W signed digits (power-of-two or mixed-radix windows), written window-major as
//      msm_tile_hist_kernel     4-byte keys; per (window, super-tile) a histogram of the keys over the coarse bins.
//   2. partition (hand-written, no library sort): column scans of the tile histograms give every (super-tile, window, bin) run
//      its exact position; msm_scatter_kernel moves (key, base index) pairs into their bin through LDS; msm_bucket_kernel sorts
//      every bin by bucket in registers and writes the per-bucket index lists (bucket starts aligned to 4 entries) and bounds;
//      msm_bigbin_* handle bins that skewed inputs overfill.  HBM-bound: 28 B per (point, window).
//   3. msm_size_*_kernel        counting sort of the buckets by size (wave-level load balance, heavy buckets first).
//   4. msm_accumulate_kernel    ONE LANE PER BUCKET for all W * nb buckets at once, in size order: gathers its affine bases and
//                               folds them into a U-form XYZZ accumulator held in VGPRs (8M+2S per point) -- the dominant
//                               kernel; the identity-base check (source.rs:50-52) is fused in;
//      msm_accumulate_heavy / msm_heavy_combine   segment-parallel path for buckets that one lane would walk too long.
//   5. msm_reduce_level_kernel  sum_k k*B_k per window by chunked running sums (levels), then
//      msm_tree_kernel          pairwise trees: plain sums of the levels' A[] and the bit decomposition of the rest;
//                               both on R-domain XYZZ records (curveu.hpp: U-form full additions).
//   6. host (msm_join.hpp)      ONE Horner pass over all partial sums, grouped by their power of two (multiexp.rs:146-154).
// The result is a group element; the reference compares/normalises projective points by value
// (ec.rs:45-85, 596-629), so parity is defined on the affine normalisation.
//
// This file is the DEVICE side: every kernel and device helper of the pipeline, and nothing else.  The host side lives in
// msm_plan.hpp (geometry, schedules and the workspace layout of a call), msm_pools.hpp (workspaces and pinned buffers),
// msm_join.hpp (the window join) and msm_host.hpp (msm_device / segsum_device: the launch sequence); the structs and limits
// both sides use are in msm_common.hpp.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "curveu.hpp"
#include "device_util.hpp"
#include "msm_common.hpp"

namespace zk {

namespace {  // one copy per translation unit (msm_g1.hip / msm_g2.hip): compiled in parallel

template <class F>
__device__ __forceinline__ Affine<F> load_affine(const Affine<F>* p) {
  // sizeof(Affine<F>) is 64 (G1) or 128 (G2): 4 / 8 x 16-byte loads
  Affine<F> r;
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint4* d = reinterpret_cast<uint4*>(&r);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(Affine<F>) / 16); ++i) d[i] = q[i];
  return r;
}

template <class T>
__device__ __forceinline__ void store_vec(T* p, const T& v) {
  const uint4* s = reinterpret_cast<const uint4*>(&v);
  uint4* d = reinterpret_cast<uint4*>(p);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 16); ++i) d[i] = s[i];
}
template <class T>
__device__ __forceinline__ T load_vec(const T* p) {
  T r;
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint4* d = reinterpret_cast<uint4*>(&r);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 16); ++i) d[i] = q[i];
  return r;
}

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

// ------------------------------------------------------------------------------------------------
// 2. PARTITION: the (window, bucket) grouping of the n * WL digits, hand-written (no library sort on the path).
//    Only GROUPING by bucket is needed (bucket membership of multiexp.rs:104-117; the order inside a bucket is irrelevant to
//    the sum), so instead of a full LSD radix sort the digits take ONE coarse and ONE fine step, both staged through LDS:
//      pass A  msm_digits_hist_kernel  scalars -> W signed digits, written window-major as 4-byte keys (bucket | sign); the
//              workgroup keeps an LDS histogram over (window, coarse bin = bucket >> lo_bits) and dumps it once per
//              super-tile of ST scalars: tile_hist[super-tile][window][bin] (u16).
//      scan    msm_colsum / msm_binscan / msm_tileoff: column-wise exclusive prefix sums of tile_hist -> for every
//              (super-tile, window, bin) the exact position of its run inside the bin's region: no atomics, no look-back.
//      pass B  msm_scatter_kernel  one workgroup per (window, super-tile): keys -> LDS histogram ranks -> the tile's
//              elements reordered by bin in LDS -> written out as contiguous runs of (key, base index) pairs.
//      pass C  msm_bucket_kernel   one workgroup per (window, coarse bin) (~2^14 elements, held in registers): LDS histogram
//              over its 2^lo_bits buckets -> bucket bounds first[] / last[] (bucket starts aligned to 4 entries so that the
//              accumulation can read its index list with 16-byte loads) -> indices placed through an LDS staging buffer and
//              written out coalesced.  Bins that outgrow registers / LDS (skewed scalars) take a two-read path.
//    HBM traffic per element: 4 B (keys) written + read, 8 B (pairs) written + read, 4 B (indices) written = 28 B, against
//    3 x 16 B for a three-pass pair sort.

// exclusive prefix sums over len <= 4 * PART_THREADS values: value(idx) -> out(idx, exclusive prefix); returns the total.
// `scratch`: 17 words of LDS.  Every thread of the 1024-thread workgroup must call it.
template <class In, class Out>
__device__ __forceinline__ uint32_t block_scan_1024(uint32_t len, uint32_t* scratch, In value, Out out) {
  constexpr uint32_t PER = 4;
  const uint32_t tid = threadIdx.x, lane = tid & 63u, wv = tid >> 6;
  uint32_t v[PER], sum = 0;
#pragma unroll
  for (uint32_t k = 0; k < PER; ++k) {
    const uint32_t idx = tid * PER + k;
    v[k] = idx < len ? value(idx) : 0u;
    sum += v[k];
  }
  uint32_t inc = sum;
#pragma unroll
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t t = __shfl_up(inc, d, 64);
    if (lane >= d) inc += t;
  }
  __syncthreads();  // scratch may still be read from a previous call
  if (lane == 63) scratch[wv] = inc;
  __syncthreads();
  if (tid == 0) {
    uint32_t run = 0;
    for (uint32_t w = 0; w < PART_THREADS / 64; ++w) {
      const uint32_t t = scratch[w];
      scratch[w] = run;
      run += t;
    }
    scratch[16] = run;
  }
  __syncthreads();
  uint32_t run = scratch[wv] + inc - sum;
#pragma unroll
  for (uint32_t k = 0; k < PER; ++k) {
    const uint32_t idx = tid * PER + k;
    if (idx < len) out(idx, run);
    run += v[k];
  }
  return scratch[16];
}

// the same over any length: chunks of 4 * PART_THREADS values with a running carry
template <class In, class Out>
__device__ __forceinline__ uint32_t block_scan_long(uint32_t len, uint32_t* scratch, In value, Out out) {
  uint32_t carry = 0;
  for (uint32_t base = 0; base < len; base += 4 * PART_THREADS) {
    const uint32_t m = len - base < 4 * PART_THREADS ? len - base : 4 * PART_THREADS;
    carry += block_scan_1024(m, scratch, [&](uint32_t x) { return value(base + x); }, [&](uint32_t x, uint32_t ex) { out(base + x, carry + ex); });
  }
  return carry;
}

// pass A.  density == nullptr: FullDensity (source.rs:80-99).  Otherwise bit i of `density` selects exponent i
// (source.rs:101-118).  scalars_mont != 0: the exponents are Fr elements in Montgomery form (what the prover holds before
// scalars_into_representations, prover.rs:89-129): the conversion into_repr() is one Montgomery reduction, fused here.
template <uint32_t RM>
__global__ void __launch_bounds__(PART_THREADS) msm_digits_hist_kernel(const uint32_t* __restrict__ scalars, uint64_t n,
                                                                       const uint32_t* __restrict__ density, MsmGeom G, uint32_t w_lo,
                                                                       uint32_t w_hi, int scalars_mont, PartGeom P, uint64_t kstride,
                                                                       uint32_t* __restrict__ keys, uint16_t* __restrict__ tile_hist,
                                                                       unsigned long long* __restrict__ err_scalar, uint64_t i_bias) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  // counters are 16 bits wide (a super-tile has at most 16384 scalars), two per LDS word: half the LDS, two workgroups per CU,
  // and the dump below is a plain copy (little endian: even cell = low half)
  uint32_t* lh = reinterpret_cast<uint32_t*>(smem);
  const uint32_t WL = w_hi - w_lo, ncell = WL * P.nbin, nword = (ncell + 1) / 2;
  for (uint32_t st = blockIdx.x; st < P.n_st; st += gridDim.x) {
    for (uint32_t t = threadIdx.x; t < nword; t += PART_THREADS) lh[t] = 0;
    __syncthreads();
    const uint64_t i_end = (uint64_t)(st + 1) * P.st < n ? (uint64_t)(st + 1) * P.st : n;
    // the next scalar of the lane is requested before the current one is worked on (~10^3 instructions): the load latency is
    // then hidden inside the lane itself, not only by the other waves
    uint4 n0 = make_uint4(0, 0, 0, 0), n1 = n0;
    {
      const uint64_t i_first = (uint64_t)st * P.st + threadIdx.x;
      if (i_first < i_end) {
        const uint4* sp = reinterpret_cast<const uint4*>(scalars + i_first * 8);
        n0 = sp[0];
        n1 = sp[1];
      }
    }
    for (uint64_t i = (uint64_t)st * P.st + threadIdx.x; i < i_end; i += PART_THREADS) {
      bool active = true;
      if (density != nullptr) active = (density[i >> 5] >> (i & 31)) & 1;
      uint32_t s[9];
      const uint4 s0 = n0, s1 = n1;
      if (i + PART_THREADS < i_end) {
        const uint4* sp = reinterpret_cast<const uint4*>(scalars + (i + PART_THREADS) * 8);
        n0 = sp[0];
        n1 = sp[1];
      }
      s[0] = s0.x; s[1] = s0.y; s[2] = s0.z; s[3] = s0.w; s[4] = s1.x; s[5] = s1.y; s[6] = s1.z; s[7] = s1.w; s[8] = 0;
      if (scalars_mont) {
        Fr f;
#pragma unroll
        for (int l = 0; l < 8; ++l) f.l[l] = s[l];
        f = to_canonical(f);
#pragma unroll
        for (int l = 0; l < 8; ++l) s[l] = f.l[l];
      }
      const uint32_t any = s[0] | s[1] | s[2] | s[3] | s[4] | s[5] | s[6] | s[7];
      if (active && (s[7] >> 30)) {
        // not a canonical FrRepr (r < 2^254): its top digit would overflow the bucket field of the key.  Reported as bad
        // arguments (the lowest such exponent index), the exponent is skipped.
        atomicMin(err_scalar, (unsigned long long)(i + i_bias));
        active = false;
      }
      if (!active || any == 0) {  // multiexp.rs:93-96: zero exponent skips its base without looking at it
        for (uint32_t wl = 0; wl < WL; ++wl) keys[(uint64_t)wl * kstride + i] = G.nb;
        continue;
      }
      // (a selected base with a non-zero exponent must not be the identity, source.rs:50-52: checked where the base is
      // loaded anyway, in accumulate_run)
      msm_scalar_digits<RM>(s, G, w_lo, w_hi < G.W ? w_hi : G.W, [&](uint32_t w, uint32_t d, uint32_t neg) {
        if (w >= w_lo && w < w_hi) {
          const uint32_t wl = w - w_lo;
          keys[(uint64_t)wl * kstride + i] = d ? ((d - 1) | neg) : G.nb;
          if (d) {
            const uint32_t cell = wl * P.nbin + ((d - 1) >> P.lo_bits);
            atomicAdd(&lh[cell >> 1], 1u << (16u * (cell & 1u)));
          }
        }
      });
    }
    __syncthreads();
    // rows are padded to an even cell count (ncell_pad) so that every row starts on a word
    uint32_t* row = reinterpret_cast<uint32_t*>(tile_hist) + (uint64_t)st * nword;
    for (uint32_t t = threadIdx.x; t < nword; t += PART_THREADS) row[t] = lh[t];
    __syncthreads();
  }
}

// pass A in two kernels (the default): a plain streaming digit kernel -- one scalar per lane, no LDS, any number of workgroups
// in flight -- and the tile histograms taken from the keys it wrote.  The fused kernel above saves the 4 bytes per (point,
// window) the histogram pass reads again, but its 1024-lane workgroups with a 61 KiB LDS histogram stream the scalars at under
// half the rate of the plain kernel (2.75 ms against 1.1 + 0.7 ms at 2^26), and a multi-GPU rank that owns a few windows pays
// the slow scalar stream in full.
template <uint32_t RM>
__global__ void __launch_bounds__(256) msm_digits_plain_kernel(const uint32_t* __restrict__ scalars, uint64_t n, const uint32_t* __restrict__ density,
                                                              MsmGeom G, uint32_t w_lo, uint32_t w_hi, int scalars_mont, uint64_t kstride,
                                                              uint32_t* __restrict__ keys, unsigned long long* __restrict__ err_scalar,
                                                              uint64_t i_bias /* index of exponent 0 of this chunk in the whole call */) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t WL = w_hi - w_lo;
  if (i >= n) {
    // the (at most three) slots between the key planes: "no bucket", so that a table-mode call can read the planes as ONE array
    if (i < kstride) for (uint32_t wl = 0; wl < WL; ++wl) keys[(uint64_t)wl * kstride + i] = G.nb;
    return;
  }
  bool active = true;
  if (density != nullptr) active = (density[i >> 5] >> (i & 31)) & 1;
  uint32_t s[9];
  const uint4* sp = reinterpret_cast<const uint4*>(scalars + i * 8);
  const uint4 s0 = sp[0], s1 = sp[1];
  s[0] = s0.x; s[1] = s0.y; s[2] = s0.z; s[3] = s0.w; s[4] = s1.x; s[5] = s1.y; s[6] = s1.z; s[7] = s1.w; s[8] = 0;
  if (scalars_mont) {
    Fr f;
#pragma unroll
    for (int l = 0; l < 8; ++l) f.l[l] = s[l];
    f = to_canonical(f);
#pragma unroll
    for (int l = 0; l < 8; ++l) s[l] = f.l[l];
  }
  const uint32_t any = s[0] | s[1] | s[2] | s[3] | s[4] | s[5] | s[6] | s[7];
  if (active && (s[7] >> 30)) {   // not a canonical FrRepr: see msm_digits_hist_kernel
    atomicMin(err_scalar, (unsigned long long)(i + i_bias));
    active = false;
  }
  if (!active || any == 0) {
    for (uint32_t wl = 0; wl < WL; ++wl) keys[(uint64_t)wl * kstride + i] = G.nb;
    return;
  }
  msm_scalar_digits<RM>(s, G, w_lo, w_hi < G.W ? w_hi : G.W, [&](uint32_t w, uint32_t d, uint32_t neg) {
    if (w >= w_lo && w < w_hi) keys[(uint64_t)(w - w_lo) * kstride + i] = d ? ((d - 1) | neg) : G.nb;
  });
}

// tile_hist[st][wl][bin] from the keys of (window wl, super-tile st): one workgroup each
__global__ void __launch_bounds__(PART_THREADS) msm_tile_hist_kernel(const uint32_t* __restrict__ keys, uint64_t n, uint64_t kstride, uint32_t nb,
                                                                     uint32_t WL, PartGeom P, uint16_t* __restrict__ tile_hist) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* lh = reinterpret_cast<uint32_t*>(smem);
  const uint32_t st = blockIdx.x % P.n_st, wl = blockIdx.x / P.n_st;
  const uint64_t i0 = (uint64_t)st * P.st;
  const uint32_t cnt = (uint32_t)(n - i0 < P.st ? n - i0 : P.st);
  for (uint32_t t = threadIdx.x; t < P.nbin; t += PART_THREADS) lh[t] = 0;
  __syncthreads();
  const uint32_t* kp = keys + (uint64_t)wl * kstride + i0;
  for (uint32_t idx = 4u * threadIdx.x; idx < cnt; idx += 4u * PART_THREADS) {
    uint32_t v[4] = {nb, nb, nb, nb};
    if (idx + 4 <= cnt) {
      const uint4 q = *reinterpret_cast<const uint4*>(kp + idx);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
      for (uint32_t e = 0; e < 4; ++e)
        if (idx + e < cnt) v[e] = kp[idx + e];
    }
#pragma unroll
    for (uint32_t e = 0; e < 4; ++e) {
      const uint32_t b = v[e] & KEY_NONE_MASK;
      if (b < nb) atomicAdd(&lh[b >> P.lo_bits], 1u);
    }
  }
  __syncthreads();
  const uint32_t ncell = WL * P.nbin, stride = (ncell + 1u) & ~1u;
  uint16_t* row = tile_hist + (uint64_t)st * stride + (uint64_t)wl * P.nbin;
  for (uint32_t t = threadIdx.x; t < P.nbin; t += PART_THREADS) row[t] = (uint16_t)lh[t];
}

// column sums of tile_hist over one chunk of rows: csum[chunk][col]
__global__ void __launch_bounds__(256) msm_colsum_kernel(const uint16_t* __restrict__ tile_hist, PartGeom P, uint32_t ncell,
                                                        uint32_t* __restrict__ csum) {
  const uint32_t col = blockIdx.x * blockDim.x + threadIdx.x, chunk = blockIdx.y;
  if (col >= ncell) return;
  const uint32_t stride = (ncell + 1u) & ~1u;
  const uint32_t r0 = chunk * P.rows_per_chunk, r1 = r0 + P.rows_per_chunk < P.n_st ? r0 + P.rows_per_chunk : P.n_st;
  uint32_t s = 0;
#pragma unroll 8
  for (uint32_t r = r0; r < r1; ++r) s += tile_hist[(uint64_t)r * stride + col];
  csum[(uint64_t)chunk * ncell + col] = s;
}

// per column: csum[chunk][col] -> exclusive prefix over the chunks, total[col] = the column sum (coalesced across columns)
__global__ void __launch_bounds__(256) msm_colscan_kernel(uint32_t* __restrict__ csum, PartGeom P, uint32_t ncell, uint32_t* __restrict__ total) {
  const uint32_t col = blockIdx.x * blockDim.x + threadIdx.x;
  if (col >= ncell) return;
  uint32_t run = 0;
  for (uint32_t ch = 0; ch < P.n_chunk; ++ch) {
    const uint32_t v = csum[(uint64_t)ch * ncell + col];
    csum[(uint64_t)ch * ncell + col] = run;
    run += v;
  }
  total[col] = run;
}

// one workgroup: bin_start[col] = elements before (window, bin) `col` in the pair array (exclusive scan of total[]),
// out_start[col] = first slot of the bin's region in the index array (every bucket start is padded to a multiple of 4
// entries: + up to 3 per bucket).
__global__ void __launch_bounds__(PART_THREADS) msm_binscan_kernel(const uint32_t* __restrict__ total, PartGeom P, uint32_t ncell, uint32_t nb,
                                                                   uint32_t* __restrict__ bin_start, uint32_t* __restrict__ out_start) {
  __shared__ uint32_t scratch[32];
  auto padded = [&](uint32_t col) {
    const uint32_t bin = col % P.nbin;
    const uint32_t nf = ((bin + 1) << P.lo_bits) <= nb ? 1u << P.lo_bits : nb - (bin << P.lo_bits);
    return (total[col] + 3u * nf + 3u) & ~3u;
  };
  const uint32_t t0 = block_scan_long(ncell, scratch, [&](uint32_t c) { return total[c]; }, [&](uint32_t c, uint32_t ex) { bin_start[c] = ex; });
  const uint32_t t1 = block_scan_long(ncell, scratch, padded, [&](uint32_t c, uint32_t ex) { out_start[c] = ex; });
  if (threadIdx.x == 0) {
    bin_start[ncell] = t0;
    out_start[ncell] = t1;
  }
}

// tile_off[row][col] = position in the pair array at which super-tile `row` writes its run of (window, bin) `col`
__global__ void __launch_bounds__(256) msm_tileoff_kernel(const uint16_t* __restrict__ tile_hist, const uint32_t* __restrict__ cbase,
                                                         const uint32_t* __restrict__ bin_start, PartGeom P, uint32_t ncell,
                                                         uint32_t* __restrict__ tile_off) {
  const uint32_t col = blockIdx.x * blockDim.x + threadIdx.x, chunk = blockIdx.y;
  if (col >= ncell) return;
  const uint32_t stride = (ncell + 1u) & ~1u;
  const uint32_t r0 = chunk * P.rows_per_chunk, r1 = r0 + P.rows_per_chunk < P.n_st ? r0 + P.rows_per_chunk : P.n_st;
  uint32_t run = bin_start[col] + cbase[(uint64_t)chunk * ncell + col];
#pragma unroll 8
  for (uint32_t r = r0; r < r1; ++r) {
    tile_off[(uint64_t)r * ncell + col] = run;
    run += tile_hist[(uint64_t)r * stride + col];
  }
}

// pass B.  One workgroup per (window wl, super-tile st): the tile's keys are ranked inside their coarse bin by LDS atomics,
// reordered by bin in LDS and written out as one contiguous run per bin at tile_off[st][wl][bin].  The pair carries the
// key (bucket | sign) and the BASE index of the exponent: base_offset + i under FullDensity, base_offset + rank(i) for a
// density map (source.rs:101-118: rank(i) = dprefix[i/32] + popc(density[i/32] & ((1 << i%32) - 1))).
__global__ void __launch_bounds__(PART_THREADS) msm_scatter_kernel(const uint32_t* __restrict__ keys, uint64_t n, uint64_t kstride, uint64_t base_offset,
                                                                   const uint32_t* __restrict__ density, const uint32_t* __restrict__ dprefix,
                                                                   uint32_t nb, uint32_t WL, PartGeom P, uint32_t xcds,
                                                                   const uint32_t* __restrict__ tile_off, uint2* __restrict__ pairs,
                                                                   uint64_t flat_stride, uint64_t table_stride) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t nbin4 = (P.nbin + 3u) & ~3u;
  uint32_t* loff = reinterpret_cast<uint32_t*>(smem);             // nbin: counts, then exclusive offsets inside the tile
  uint32_t* delta = loff + nbin4;                                 // nbin: tile_off[bin] - loff[bin] (mod 2^32)
  uint32_t* scratch = delta + nbin4;                              // 32 words
  uint2* staging = reinterpret_cast<uint2*>(scratch + 32);        // st pairs
  // Workgroups are dealt to the XCDs round-robin by block id; runs of one bin written by CONSECUTIVE super-tiles are adjacent
  // in memory, so consecutive super-tiles are given to the same XCD (block id b -> XCD b % xcds takes a contiguous range of
  // super-tiles) and their partial lines merge in that XCD's L2 instead of leaving it one by one.
  uint32_t st, wl;
  {
    const uint32_t per = P.n_st / xcds;  // super-tiles per XCD in the remapped part
    const uint32_t body = per * xcds;    // the first `body` super-tiles are remapped, the remainder keeps the plain order
    const uint32_t b = blockIdx.x;
    if (per != 0 && b < body * WL) {
      const uint32_t x = b % xcds, j = b / xcds;
      st = x * per + j % per;
      wl = j / per;
    } else {
      const uint32_t r = b - body * WL, rem = P.n_st - body;
      st = body + r % rem;
      wl = r / rem;
    }
  }
  const uint64_t i0 = (uint64_t)st * P.st;
  const uint32_t cnt = (uint32_t)(n - i0 < P.st ? n - i0 : P.st);
  for (uint32_t t = threadIdx.x; t < P.nbin; t += PART_THREADS) loff[t] = 0;
  __syncthreads();
  // lane t holds keys 4 * (k * 1024 + t) .. + 3: one 16-byte load (the key planes are kstride = 4 * ceil(n / 4) apart, tiles are
  // multiples of 1024: every tile starts on 16 bytes)
  uint32_t key[PART_MAX_EB], rank[PART_MAX_EB];
  const uint32_t* kp = keys + (uint64_t)wl * kstride + i0;
  const bool wide = true;
#pragma unroll
  for (uint32_t k4 = 0; k4 < PART_MAX_EB / 4; ++k4) {
    const uint32_t idx = 4u * (k4 * PART_THREADS + threadIdx.x);
    uint32_t v[4] = {nb, nb, nb, nb};
    if (wide && idx + 4 <= cnt) {
      const uint4 q = *reinterpret_cast<const uint4*>(kp + idx);
      v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
    } else {
#pragma unroll
      for (uint32_t e = 0; e < 4; ++e)
        if (idx + e < cnt) v[e] = kp[idx + e];
    }
#pragma unroll
    for (uint32_t e = 0; e < 4; ++e) {
      key[4 * k4 + e] = v[e];
      rank[4 * k4 + e] = 0;
      const uint32_t b = v[e] & KEY_NONE_MASK;
      if (b < nb) rank[4 * k4 + e] = atomicAdd(&loff[b >> P.lo_bits], 1u);
    }
  }
  __syncthreads();
  const uint32_t* toff = tile_off + ((uint64_t)st * WL + wl) * P.nbin;
  const uint32_t total = block_scan_1024(P.nbin, scratch, [&](uint32_t x) { return loff[x]; },
                                         [&](uint32_t x, uint32_t ex) { loff[x] = ex; delta[x] = toff[x] - ex; });
  __syncthreads();
#pragma unroll
  for (uint32_t k4 = 0; k4 < PART_MAX_EB / 4; ++k4) {
#pragma unroll
    for (uint32_t e = 0; e < 4; ++e) {
      const uint32_t k = 4 * k4 + e;
      const uint32_t idx = 4u * (k4 * PART_THREADS + threadIdx.x) + e;
      const uint32_t b = key[k] & KEY_NONE_MASK;
      if (idx < cnt && b < nb) {
        uint64_t i = i0 + idx, tw = 0;
        if (flat_stride != 0) {  // table mode: position = window * flat_stride + exponent; the window's copy of the bases starts at window * table_stride
          tw = i / flat_stride;
          i -= tw * flat_stride;
          tw *= table_stride;
        }
        uint64_t bi = base_offset + i;
        if (density != nullptr) {
          const uint32_t wd = density[i >> 5];
          bi = base_offset + dprefix[i >> 5] + __popc(wd & ((1u << (i & 31)) - 1u));
        }
        bi += tw;
        staging[loff[b >> P.lo_bits] + rank[k]] = make_uint2(key[k], (uint32_t)bi);
      }
    }
  }
  __syncthreads();
  for (uint32_t p = threadIdx.x; p < total; p += PART_THREADS) {
    const uint2 e = staging[p];
    pairs[(uint64_t)(p + delta[(e.x & KEY_NONE_MASK) >> P.lo_bits])] = e;
  }
}

// pass C.  One workgroup per (window wl, coarse bin): its pairs [bin_start[col], bin_start[col + 1]) are grouped by bucket.
//   first[id] / last[id] (id = wl * nb + bucket) delimit the bucket's index list inside `vals`; every list starts at a
//   multiple of 4 entries (16-byte loads in the accumulation; the padding slots are never consumed).
//   vals entry = base index | SIGN_BIT for a negative digit.
__global__ void __launch_bounds__(PART_THREADS) msm_bucket_kernel(const uint2* __restrict__ pairs, const uint32_t* __restrict__ bin_start,
                                                                  const uint32_t* __restrict__ out_start, uint32_t nb, PartGeom P,
                                                                  uint32_t stage_cap, uint32_t* __restrict__ first, uint32_t* __restrict__ last,
                                                                  uint32_t* __restrict__ vals) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const uint32_t nfmax = 1u << P.lo_bits;
  const uint32_t nfl = nfmax < 4 ? 4 : nfmax;            // (keeps `staging` 16-byte aligned)
  uint32_t* hist = reinterpret_cast<uint32_t*>(smem);   // nfmax
  uint32_t* start = hist + nfl;                          // nfmax
  uint32_t* scratch = start + nfl;                       // 32
  uint32_t* staging = scratch + 32;                      // stage_cap
  const uint32_t col = blockIdx.x, wl = col / P.nbin, bin = col % P.nbin;
  const uint32_t beg = bin_start[col], cnt = bin_start[col + 1] - beg;
  const uint32_t ob = out_start[col];
  const uint32_t nf = (bin + 1) << P.lo_bits <= nb ? nfmax : nb - (bin << P.lo_bits);
  const uint32_t fmask = nfmax - 1u;
  for (uint32_t t = threadIdx.x; t < nfmax; t += PART_THREADS) hist[t] = 0;
  __syncthreads();
  if (cnt > PART_EC * PART_THREADS) return;  // a BIG bin (skewed exponents, or very large n): msm_bigbin_* kernels, many workgroups
  uint32_t val[PART_EC], fr[PART_EC];  // fr = fine bucket | rank << PART_LO_MAX
#pragma unroll
  for (uint32_t k = 0; k < PART_EC; ++k) {
    const uint32_t idx = k * PART_THREADS + threadIdx.x;
    val[k] = 0;
    fr[k] = 0;
    if (idx < cnt) {
      const uint2 e = pairs[(uint64_t)beg + idx];
      const uint32_t f = e.x & fmask;
      val[k] = e.y | (e.x & SIGN_BIT);
      fr[k] = f | (atomicAdd(&hist[f], 1u) << PART_LO_MAX);
    }
  }
  __syncthreads();
  const uint32_t padded = block_scan_1024(nf, scratch, [&](uint32_t x) { return (hist[x] + 3u) & ~3u; },
                                          [&](uint32_t x, uint32_t ex) { start[x] = ex; });
  __syncthreads();
  const uint32_t id0 = wl * nb + (bin << P.lo_bits);
  for (uint32_t t = threadIdx.x; t < nf; t += PART_THREADS) {
    first[id0 + t] = ob + start[t];
    last[id0 + t] = ob + start[t] + hist[t];
  }
  if (padded <= stage_cap) {
#pragma unroll
    for (uint32_t k = 0; k < PART_EC; ++k) {
      const uint32_t idx = k * PART_THREADS + threadIdx.x;
      if (idx < cnt) staging[start[fr[k] & ((1u << PART_LO_MAX) - 1u)] + (fr[k] >> PART_LO_MAX)] = val[k];
    }
    __syncthreads();
    // 16-byte stores; `ob` and `padded` are multiples of 4
    uint4* dst = reinterpret_cast<uint4*>(vals + ob);
    const uint4* src = reinterpret_cast<const uint4*>(staging);
    for (uint32_t q = threadIdx.x; q < padded / 4; q += PART_THREADS) dst[q] = src[q];
  } else {
#pragma unroll
    for (uint32_t k = 0; k < PART_EC; ++k) {
      const uint32_t idx = k * PART_THREADS + threadIdx.x;
      if (idx < cnt) vals[(uint64_t)ob + start[fr[k] & ((1u << PART_LO_MAX) - 1u)] + (fr[k] >> PART_LO_MAX)] = val[k];
    }
  }
}

// BIG bins: more elements than one workgroup holds in registers.  Prover-like exponents do this -- a Groth16 witness is full of
// 0 / 1 / small values, so window 0 sends a large share of ALL points into the first few buckets, i.e. into one bin -- and so does
// a uniform input at n > 2^26.  Such a bin is cut into SEGMENTS of PART_EC * 1024 elements, one workgroup each:
//   msm_bigbin_plan_kernel   (one workgroup) the list of big bins and the prefix of their segment counts
//   msm_bigbin_count_kernel  every segment adds its LDS histogram over the bin's buckets to gcnt[bucket id]
//   msm_bigbin_place_kernel  every segment derives the bucket starts from gcnt (scan, 4-entry aligned like the small bins),
//                            reserves its share of each bucket with ONE atomic per non-empty bucket (gcur) and writes its
//                            indices; segment 0 of a bin also writes first[] / last[].
// A fixed grid strides over the segments -- the host never reads the plan back -- and idle workgroups exit at once.

__global__ void __launch_bounds__(PART_THREADS) msm_bigbin_plan_kernel(const uint32_t* __restrict__ bin_start, uint32_t ncell,
                                                                       uint32_t* __restrict__ big_col, uint32_t* __restrict__ big_seg_off,
                                                                       BigPlan* __restrict__ plan) {
  __shared__ uint32_t scratch[32];
  auto cnt_of = [&](uint32_t col) { return bin_start[col + 1] - bin_start[col]; };
  // compact the big bins, then the prefix of their segment counts
  const uint32_t n_big = block_scan_long(ncell, scratch, [&](uint32_t c) { return cnt_of(c) > BIG_SEG ? 1u : 0u; },
                                         [&](uint32_t c, uint32_t ex) { if (cnt_of(c) > BIG_SEG) big_col[ex] = c; });
  __syncthreads();
  const uint32_t n_seg = block_scan_long(n_big, scratch, [&](uint32_t k) { return (cnt_of(big_col[k]) + BIG_SEG - 1) / BIG_SEG; },
                                         [&](uint32_t k, uint32_t ex) { big_seg_off[k] = ex; });
  if (threadIdx.x == 0) {
    plan->n_big = n_big;
    plan->total_seg = n_seg;
  }
}

// The four scans above in ONE single-workgroup launch, for SHORT calls (n_st * ncell small: a 2^16-point call has 16 super-tiles x ~2000
// columns): a call of 0.4 - 0.6 ms pays ~5 us for every launch, however little it does.  Also clears the size histogram of the
// bucket order (one memset less) and writes the (empty-or-not) big-bin plan.
__global__ void __launch_bounds__(PART_THREADS) msm_scan_small_kernel(const uint16_t* __restrict__ tile_hist, PartGeom P, uint32_t ncell, uint32_t nb,
                                                                      uint32_t* __restrict__ col_total, uint32_t* __restrict__ bin_start,
                                                                      uint32_t* __restrict__ out_start, uint32_t* __restrict__ tile_off,
                                                                      uint32_t* __restrict__ size_hist, uint32_t* __restrict__ big_col,
                                                                      uint32_t* __restrict__ big_seg_off, BigPlan* __restrict__ plan) {
  __shared__ uint32_t scratch[32];
  const uint32_t stride = (ncell + 1u) & ~1u;
  for (uint32_t t = threadIdx.x; t < MSM_SIZE_BINS; t += PART_THREADS) size_hist[t] = 0;
  for (uint32_t col = threadIdx.x; col < ncell; col += PART_THREADS) {
    uint32_t s = 0;
    for (uint32_t r = 0; r < P.n_st; ++r) s += tile_hist[(uint64_t)r * stride + col];
    col_total[col] = s;
  }
  __syncthreads();   // (global writes of this workgroup are visible to it after the barrier)
  auto padded = [&](uint32_t col) {
    const uint32_t bin = col % P.nbin;
    const uint32_t nf = ((bin + 1) << P.lo_bits) <= nb ? 1u << P.lo_bits : nb - (bin << P.lo_bits);
    return (col_total[col] + 3u * nf + 3u) & ~3u;
  };
  const uint32_t t0 = block_scan_long(ncell, scratch, [&](uint32_t c) { return col_total[c]; }, [&](uint32_t c, uint32_t ex) { bin_start[c] = ex; });
  const uint32_t t1 = block_scan_long(ncell, scratch, padded, [&](uint32_t c, uint32_t ex) { out_start[c] = ex; });
  if (threadIdx.x == 0) {
    bin_start[ncell] = t0;
    out_start[ncell] = t1;
  }
  __syncthreads();
  for (uint32_t col = threadIdx.x; col < ncell; col += PART_THREADS) {
    uint32_t run = bin_start[col];
    for (uint32_t r = 0; r < P.n_st; ++r) {
      tile_off[(uint64_t)r * ncell + col] = run;
      run += tile_hist[(uint64_t)r * stride + col];
    }
  }
  // the big-bin plan (msm_bigbin_plan_kernel)
  auto cnt_of = [&](uint32_t col) { return bin_start[col + 1] - bin_start[col]; };
  const uint32_t n_big = block_scan_long(ncell, scratch, [&](uint32_t c) { return cnt_of(c) > BIG_SEG ? 1u : 0u; },
                                         [&](uint32_t c, uint32_t ex) { if (cnt_of(c) > BIG_SEG) big_col[ex] = c; });
  __syncthreads();
  const uint32_t n_seg = block_scan_long(n_big, scratch, [&](uint32_t k) { return (cnt_of(big_col[k]) + BIG_SEG - 1) / (BIG_SEG); },
                                         [&](uint32_t k, uint32_t ex) { big_seg_off[k] = ex; });
  if (threadIdx.x == 0) {
    plan->n_big = n_big;
    plan->total_seg = n_seg;
  }
}

// (big bin, segment) of workgroup b: the last k with big_seg_off[k] <= b
__device__ __forceinline__ bool bigbin_locate(const BigPlan* plan, const uint32_t* big_col, const uint32_t* big_seg_off, uint32_t b,
                                              uint32_t* col, uint32_t* seg) {
  if (b >= plan->total_seg) return false;
  uint32_t lo = 0, hi = plan->n_big;
  while (hi - lo > 1) {
    const uint32_t mid = (lo + hi) >> 1;
    if (big_seg_off[mid] <= b) lo = mid;
    else hi = mid;
  }
  *col = big_col[lo];
  *seg = b - big_seg_off[lo];
  return true;
}

__global__ void __launch_bounds__(PART_THREADS) msm_bigbin_count_kernel(const uint2* __restrict__ pairs, const uint32_t* __restrict__ bin_start,
                                                                        const BigPlan* __restrict__ plan, const uint32_t* __restrict__ big_col,
                                                                        const uint32_t* __restrict__ big_seg_off, uint32_t nb, PartGeom P,
                                                                        uint32_t* __restrict__ gcnt) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint32_t* hist = reinterpret_cast<uint32_t*>(smem);
  for (uint32_t b = blockIdx.x;; b += gridDim.x) {   // a fixed grid strides over the segments (their number is only known on the device)
    uint32_t col, seg;
    if (!bigbin_locate(plan, big_col, big_seg_off, b, &col, &seg)) return;
    const uint32_t nfmax = 1u << P.lo_bits, fmask = nfmax - 1u;
    const uint32_t wl = col / P.nbin, bin = col % P.nbin;
    const uint32_t beg = bin_start[col] + seg * BIG_SEG, end = bin_start[col + 1];
    const uint32_t cnt = end - beg < BIG_SEG ? end - beg : BIG_SEG;
    for (uint32_t t = threadIdx.x; t < nfmax; t += PART_THREADS) hist[t] = 0;
    __syncthreads();
    for (uint32_t idx = threadIdx.x; idx < cnt; idx += PART_THREADS) atomicAdd(&hist[pairs[(uint64_t)beg + idx].x & fmask], 1u);
    __syncthreads();
    const uint32_t id0 = wl * nb + (bin << P.lo_bits);
    for (uint32_t t = threadIdx.x; t < nfmax; t += PART_THREADS)
      if (hist[t]) atomicAdd(&gcnt[id0 + t], hist[t]);
    __syncthreads();
  }
}

__global__ void __launch_bounds__(PART_THREADS) msm_bigbin_place_kernel(const uint2* __restrict__ pairs, const uint32_t* __restrict__ bin_start,
                                                                        const uint32_t* __restrict__ out_start, const BigPlan* __restrict__ plan,
                                                                        const uint32_t* __restrict__ big_col, const uint32_t* __restrict__ big_seg_off,
                                                                        uint32_t nb, PartGeom P, int staged, const uint32_t* __restrict__ gcnt,
                                                                        uint32_t* __restrict__ gcur, uint32_t* __restrict__ first,
                                                                        uint32_t* __restrict__ last, uint32_t* __restrict__ vals) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  for (uint32_t blk = blockIdx.x;; blk += gridDim.x) {
  uint32_t col, seg;
  if (!bigbin_locate(plan, big_col, big_seg_off, blk, &col, &seg)) return;
  const uint32_t nfmax = 1u << P.lo_bits, fmask = nfmax - 1u;
  const uint32_t nfl = nfmax < 4 ? 4 : nfmax;
  uint32_t* hist = reinterpret_cast<uint32_t*>(smem);   // this segment's count per bucket, then its reserved base inside the bucket
  uint32_t* start = hist + nfl;                          // the bucket's first slot relative to the bin's region
  uint32_t* scratch = start + nfl;                       // 32
  uint32_t* lstart = scratch + 32;                       // staged: the bucket's first slot inside this segment's staging area, then its length
  uint32_t* llen = lstart + nfl;
  uint32_t* staging = llen + nfl;                        // staged: BIG_SEG indices
  const uint32_t wl = col / P.nbin, bin = col % P.nbin;
  const uint32_t beg = bin_start[col] + seg * BIG_SEG, end = bin_start[col + 1];
  const uint32_t cnt = end - beg < BIG_SEG ? end - beg : BIG_SEG;
  const uint32_t ob = out_start[col];
  const uint32_t nf = (bin + 1) << P.lo_bits <= nb ? nfmax : nb - (bin << P.lo_bits);
  const uint32_t id0 = wl * nb + (bin << P.lo_bits);
  for (uint32_t t = threadIdx.x; t < nfmax; t += PART_THREADS) hist[t] = 0;
  __syncthreads();
  uint32_t val[PART_EC], fr[PART_EC];
#pragma unroll
  for (uint32_t k = 0; k < PART_EC; ++k) {
    const uint32_t idx = k * PART_THREADS + threadIdx.x;
    val[k] = 0;
    fr[k] = 0;
    if (idx < cnt) {
      const uint2 e = pairs[(uint64_t)beg + idx];
      const uint32_t f = e.x & fmask;
      val[k] = e.y | (e.x & SIGN_BIT);
      fr[k] = f | (atomicAdd(&hist[f], 1u) << PART_LO_MAX);   // rank < 2^15 (a segment has 2^15 elements): fits above the 12 bucket bits
    }
  }
  __syncthreads();
  block_scan_1024(nf, scratch, [&](uint32_t x) { return (gcnt[id0 + x] + 3u) & ~3u; }, [&](uint32_t x, uint32_t ex) { start[x] = ex; });
  if (staged) block_scan_1024(nf, scratch, [&](uint32_t x) { return hist[x]; }, [&](uint32_t x, uint32_t ex) { lstart[x] = ex; });
  __syncthreads();
  for (uint32_t t = threadIdx.x; t < nf; t += PART_THREADS) {
    if (seg == 0) {
      first[id0 + t] = ob + start[t];
      last[id0 + t] = ob + start[t] + gcnt[id0 + t];
    }
    const uint32_t mine = hist[t];
    if (staged) llen[t] = mine;
    hist[t] = mine ? atomicAdd(&gcur[id0 + t], mine) : 0u;   // this segment's base inside bucket t
  }
  __syncthreads();
  if (staged) {
    // the segment's indices grouped by bucket in LDS, then every bucket's run written by one wave: contiguous stores
    // (64 lanes x 4 B) instead of one 4-byte store per lane all over the bin's region
#pragma unroll
    for (uint32_t k = 0; k < PART_EC; ++k) {
      const uint32_t idx = k * PART_THREADS + threadIdx.x;
      if (idx < cnt) staging[lstart[fr[k] & ((1u << PART_LO_MAX) - 1u)] + (fr[k] >> PART_LO_MAX)] = val[k];
    }
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    for (uint32_t f = wv; f < nf; f += PART_THREADS / 64) {
      const uint32_t len = llen[f];
      const uint32_t* src = staging + lstart[f];
      uint32_t* dst = vals + (uint64_t)ob + start[f] + hist[f];
      for (uint32_t q = lane; q < len; q += 64) dst[q] = src[q];
    }
    __syncthreads();
    continue;
  }
#pragma unroll
  for (uint32_t k = 0; k < PART_EC; ++k) {
    const uint32_t idx = k * PART_THREADS + threadIdx.x;
    if (idx < cnt) {
      const uint32_t f = fr[k] & ((1u << PART_LO_MAX) - 1u);
      vals[(uint64_t)ob + start[f] + hist[f] + (fr[k] >> PART_LO_MAX)] = val[k];
    }
  }
  __syncthreads();
  }
}


// 3b. buckets ordered by size (descending) so that the 64 lanes of a wave own buckets of (nearly) equal length --
//     bucket sizes are Poisson distributed and a wave runs as long as its longest lane -- and so that the few very
//     long buckets of a skewed input come first.  A counting sort on the size (exact below 2048, then in steps of
//     2048): histogram, suffix scan, scatter; the order inside a bin is irrelevant.
__device__ __forceinline__ uint32_t msm_size_bin(uint32_t sz) {
  uint32_t hi = sz >> 11;
  return sz < 2048 ? sz : 2048 + (hi < 2047 ? hi : 2047);
}
__global__ void __launch_bounds__(1024) msm_size_hist_kernel(const uint32_t* __restrict__ first, const uint32_t* __restrict__ last,
                                                            uint32_t n_buckets, uint32_t* __restrict__ hist) {
  __shared__ uint32_t lh[MSM_SIZE_BINS];
  for (uint32_t t = threadIdx.x; t < MSM_SIZE_BINS; t += blockDim.x) lh[t] = 0;
  __syncthreads();
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < n_buckets; b += gridDim.x * blockDim.x)
    atomicAdd(&lh[msm_size_bin(last[b] - first[b])], 1u);
  __syncthreads();
  for (uint32_t t = threadIdx.x; t < MSM_SIZE_BINS; t += blockDim.x)
    if (lh[t]) atomicAdd(&hist[t], lh[t]);
}
// offs[bin] = number of buckets in larger bins (in place over hist); one workgroup
__global__ void __launch_bounds__(1024) msm_size_scan_kernel(uint32_t* __restrict__ hist) {
  __shared__ uint32_t part[1024];
  constexpr uint32_t PER = MSM_SIZE_BINS / 1024;
  uint32_t v[PER], sum = 0;
  for (uint32_t k = 0; k < PER; ++k) { v[k] = hist[threadIdx.x * PER + k]; sum += v[k]; }
  part[threadIdx.x] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {  // inclusive suffix sums
    uint32_t add = threadIdx.x + d < 1024 ? part[threadIdx.x + d] : 0;
    __syncthreads();
    part[threadIdx.x] += add;
    __syncthreads();
  }
  uint32_t run = part[threadIdx.x] - sum;  // buckets in the bins of higher threads
  for (int k = (int)PER - 1; k >= 0; --k) { hist[threadIdx.x * PER + k] = run; run += v[k]; }
}
constexpr uint32_t MSM_SCATTER_PER = 4;  // buckets per lane
__global__ void __launch_bounds__(1024) msm_size_scatter_kernel(const uint32_t* __restrict__ first, const uint32_t* __restrict__ last,
                                                               uint32_t n_buckets, uint32_t* __restrict__ offs, uint32_t* __restrict__ order,
                                                               uint32_t* __restrict__ sizes_sorted) {
  __shared__ uint32_t cnt[MSM_SIZE_BINS];
  __shared__ uint32_t base[MSM_SIZE_BINS];
  for (uint32_t t = threadIdx.x; t < MSM_SIZE_BINS; t += blockDim.x) cnt[t] = 0;
  __syncthreads();
  uint32_t sz[MSM_SCATTER_PER], rank[MSM_SCATTER_PER];
  const uint32_t b0 = blockIdx.x * (blockDim.x * MSM_SCATTER_PER) + threadIdx.x;
#pragma unroll
  for (uint32_t k = 0; k < MSM_SCATTER_PER; ++k) {
    uint32_t b = b0 + k * blockDim.x;
    if (b < n_buckets) {
      sz[k] = last[b] - first[b];
      rank[k] = atomicAdd(&cnt[msm_size_bin(sz[k])], 1u);
    }
  }
  __syncthreads();
  for (uint32_t t = threadIdx.x; t < MSM_SIZE_BINS; t += blockDim.x)
    if (cnt[t]) base[t] = atomicAdd(&offs[t], cnt[t]);
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < MSM_SCATTER_PER; ++k) {
    uint32_t b = b0 + k * blockDim.x;
    if (b < n_buckets) {
      uint32_t pos = base[msm_size_bin(sz[k])] + rank[k];
      order[pos] = b;
      sizes_sorted[pos] = sz[k];
    }
  }
}

// Bucket sums and everything derived from them (segment sums, running sums, tree sums, window sums) are XYZZ records in the R
// domain of curveu.hpp (canonical coordinates in the 2^261 domain, 128 B for G1 and 256 B for G2): additions run on U-form
// arithmetic -- 1.33 x the product rate of the memory format (tools/ubench_fieldmul.hip) and one reduction per Fq2 component.
template <class F>
__host__ __device__ __forceinline__ void rec_add(XYZZ<F>& a, const XYZZ<F>& b) {
  if (b.is_zero()) return;
  if (a.is_zero()) { a = b; return; }
  auto ua = xyzzr_load(a);
  xyzzr_add(ua, xyzzr_load(b));
  a = xyzzr_store(ua);
}
template <class F>
__host__ __device__ __forceinline__ XYZZ<F> rec_to_std(const XYZZ<F>& r) { return xyzzr_to_std(r); }

// A4: the index list starts on a multiple of 4 entries, is walked with stride 1 and its padding slots are readable (the
// lists the partition writes): a lane reads its indices FOUR AT A TIME with one 16-byte load.  Read one by
// one, a lane touches each 128-byte line of its list 32 times, ~10^4 instructions apart, and by then the line has usually
// left the caches (64 lanes x 16 waves x 32 CUs share an L2 that 52 GB of bases stream through): 8 touches instead of 32.
template <class F>
struct BucketAcc { using type = XYZZU<FqParams>; };
template <>
struct BucketAcc<Fq2> { using type = XYZZU2; };

// acc += the signed points of one index list.  The accumulator is the caller's: zero for a fresh bucket, xyzzu_from_r(record)
// for a bucket carried from an earlier chunk of a streamed multiexp (msm_accumulate_kernel<.., CARRY>).
// The bases are raw affine records with CANONICAL coordinates (< p), as every producer of such records writes them (the decoders of
// codec.hip, batch_normalize, the reference's own vectors); nothing checks that at upload, and xyzzu_add_mixed / xyzzu_from_affine_pair
// state it as their precondition: their lazy subtractions are sized for it, and the pair start finds two points with the same x by
// comparing the loaded words (a record holding x + p instead of x would be added as a different x: a wrong bucket, no error).
// PAIR_START (G1): a run of at least two entries that meets an EMPTY accumulator opens with xyzzu_from_affine_pair (curveu.hpp: 855 mads
// for the first two points where the copy into the empty accumulator and a full mixed addition cost 1791) and the loop takes over at the
// third entry.  The gathers keep their order: point 2 is issued as ever, point 3 is in flight before the pair arithmetic starts.  An
// identity record among the first two leaves everything to the loop, from entry j, with its skip / error report.  The CARRY launches
// do not set it: a lane whose carried record is not empty would enter the loop two entries behind its neighbours and the A4 reload
// below would no longer be uniform over the wave.
template <class F, bool A4 = false, bool PAIR_START = false>
__device__ __forceinline__ typename BucketAcc<F>::type accumulate_run(typename BucketAcc<F>::type acc, const Affine<F>* __restrict__ bases, const uint32_t* __restrict__ vals,
                                               uint32_t j, uint32_t e, uint32_t stride, bool skip_zero, unsigned long long* __restrict__ err_base) {
  // the all-zero record is the point at infinity (no curve point has y == 0).  skip_zero (dense mode, powersoftau's
  // dense_multiexp): it adds nothing.  Otherwise it is the reference's UnexpectedIdentity (source.rs:50-52: a selected base
  // with a non-zero exponent): the lowest such BASE index is reported and the record skipped.
  // (precondition: j < e -- the callers deal with an empty list before they set an accumulator up)
  // The gather of point k+1 is issued, as back-to-back 16-byte loads, before the ~2200 (G2: ~7000) ALU instructions of
  // addition k: the loads of a record then hit the same 128-byte line while it is still in cache (left to the
  // scheduler they drift apart to their uses and the line is fetched more than once: +22 % HBM traffic).
  // A4: this group of four indices, rotated so that q.x is the current one.  (A second group loaded one step ahead was
  // measured too: it costs four more VGPRs -- 129, one over the 128 that allow four waves per SIMD.)
  uint4 q = make_uint4(0, 0, 0, 0);
  uint32_t v;
  if constexpr (A4) {
    q = *reinterpret_cast<const uint4*>(vals + j);
    v = q.x;
  } else {
    v = vals[j];
  }
  Affine<F> p = load_affine(bases + (v & ~SIGN_BIT));
  bool more_left = true;
  if constexpr (PAIR_START && std::is_same<F, Fq>::value) {
    if (acc.is_zero() && j + stride < e) {
      uint4 q2 = q;
      const uint32_t j2 = j + stride, j3 = j2 + stride;
      const bool more3 = j3 < e;
      uint32_t v2, v3 = 0;
      if constexpr (A4) {
        q2.x = q2.y; q2.y = q2.z; q2.z = q2.w;   // j is a multiple of 4 and the stride is 1: entries 2 and 3 are in the group loaded above
        v2 = q2.x;
      } else {
        v2 = vals[j2];
      }
      const Affine<F> p2 = load_affine(bases + (v2 & ~SIGN_BIT));
      Affine<F> p3 = p2;
      if constexpr (A4) {
        q2.x = q2.y; q2.y = q2.z; q2.z = q2.w;
        v3 = q2.x;
        if (more3) p3 = load_affine(bases + (v3 & ~SIGN_BIT));
      } else if (more3) {
        v3 = vals[j3];
        p3 = load_affine(bases + (v3 & ~SIGN_BIT));
      }
      if (!p.y.is_zero() && !p2.y.is_zero()) {
        acc = xyzzu_from_affine_pair(p.x, p.y, (v & SIGN_BIT) != 0, p2.x, p2.y, (v2 & SIGN_BIT) != 0);
        more_left = more3;
        q = q2;
        v = v3;
        p = p3;
        j = j3;
      }
    }
  }
  if (more_left) for (;;) {
    const uint32_t jn = j + stride;
    const bool more = jn < e;
    uint32_t vn = 0;
    Affine<F> pn = p;
    if constexpr (A4) {
      if ((jn & 3u) == 0) {  // uniform over the wave: every lane started on a multiple of 4, or (PAIR_START) two entries further -- all lanes with
                             // a second entry alike, save one that met an identity record among its first two (an error, or dense mode's rare skip)
        if (more) q = *reinterpret_cast<const uint4*>(vals + jn);
      } else {
        q.x = q.y; q.y = q.z; q.z = q.w;
      }
      vn = q.x;
      if (more) pn = load_affine(bases + (vn & ~SIGN_BIT));
    } else if (more) {
      vn = vals[jn];
      pn = load_affine(bases + (vn & ~SIGN_BIT));
    }
    if (!p.y.is_zero()) {
      if constexpr (std::is_same<F, Fq>::value) xyzzu_add_mixed(acc, p.x, p.y, (v & SIGN_BIT) != 0);
      else xyzzu2_add_mixed(acc, p.x, p.y, (v & SIGN_BIT) != 0);
    } else if (!skip_zero) {
      atomicMin(err_base, (unsigned long long)(v & ~SIGN_BIT));
    }
    if (!more) break;
    v = vn;
    p = pn;
    j = jn;
  }
  return acc;
}

// 4a. heavy buckets (longer than `heavy`: skewed scalars such as the many 0/1 witnesses of a Groth16 prover --
//     every scalar equal to 1 lands in bucket 1 of window 0 -- and the short top window).  A heavy bucket is cut
//     into segments of MSM_HEAVY_SEG entries; every segment is one wave (64 strided partial sums + an
//     LDS tree) and a second kernel adds the segment sums of each bucket, so even a bucket holding a third
//     of all points is spread over thousands of workgroups.  Because `order` is sorted by size, the heavy
//     buckets are order[0..H): msm_heavy_plan_kernel scans ceil(size / SEG) over that prefix.

// item_off: hb + 2 words.  [0 .. H]: exclusive scan of the segment counts over the H leading entries of the size order that can be
// heavy, [H] = the number of segments; [hb + 1] = H.  The size order is a counting sort over msm_size_bin -- descending in the BIN, not
// inside a bin -- so H = the entries whose bin is at least the bin of heavy + 1 (a binary search), and the exact test runs on those
// only: uniform exponents have H = 0 and the three launches of the heavy path cost their start-up (0.02 ms instead of the 0.06 ms of
// a scan over all hb entries).
__global__ void __launch_bounds__(1024) msm_heavy_plan_kernel(const uint32_t* __restrict__ sizes_sorted, uint32_t hb, uint32_t heavy, uint32_t seg,
                                                             uint32_t* __restrict__ item_off /* hb + 2 */) {
  __shared__ uint32_t scratch[32];
  const uint32_t bin_min = msm_size_bin(heavy == 0xffffffffu ? heavy : heavy + 1);
  uint32_t lo = 0, hi = hb;  // first index whose bin is below bin_min (uniform over the workgroup: every lane walks the same path)
  while (lo < hi) {
    const uint32_t mid = (lo + hi) >> 1;
    if (msm_size_bin(sizes_sorted[mid]) >= bin_min) lo = mid + 1;
    else hi = mid;
  }
  const uint32_t H = lo;
  const uint32_t tot = block_scan_long(H, scratch, [&](uint32_t i) {
    const uint32_t sz = sizes_sorted[i];
    return sz > heavy ? (sz + seg - 1) / seg : 0u;
  }, [&](uint32_t i, uint32_t ex) { item_off[i] = ex; });
  if (threadIdx.x == 0) {
    item_off[H] = tot;
    item_off[hb + 1] = H;
  }
}

// Sum of the 64 lanes' partial sums of a one-wave workgroup, by QUAD additions (curveu.hpp: xyzzr_add_quad): the sums go to LDS once,
// then quad q = lane / 4 adds the pairs (e, e + s) for e = q, q + 16, ..: 2 + 1 + 1 + 1 + 1 + 1 quad additions in sequence instead of
// six one-lane additions, each 2.4 x (G2: 3 x) shorter.  Every lane of quad 0 -- lane 0 among them -- returns the total.
// `sh`: 64 entries; all 64 lanes must call it (it synchronises the workgroup).
template <class U>
__device__ __forceinline__ U wave_sum_quads(U a, U* sh) {
  sh[threadIdx.x] = a;
  __syncthreads();
  const uint32_t q = threadIdx.x >> 2, role = threadIdx.x & 3u;
  for (uint32_t s = 32; s > 0; s >>= 1) {
    for (uint32_t e = q; e < s; e += 16) {       // (uniform over a quad)
      const U x = xyzzr_add_quad(sh[e], sh[e + s], role);
      if (role == 0) sh[e] = x;
    }
    __syncthreads();
  }
  return sh[0];
}

template <class F>
__global__ void __launch_bounds__(MSM_HEAVY_LANES) msm_accumulate_heavy_kernel(const Affine<F>* __restrict__ bases, const uint32_t* __restrict__ vals,
                                                                  const uint32_t* __restrict__ first, const uint32_t* __restrict__ last,
                                                                  const uint32_t* __restrict__ order, const uint32_t* __restrict__ item_off,
                                                                  uint32_t hb, uint32_t seg, XYZZ<F>* __restrict__ seg_sums, int skip_zero,
                                                                  unsigned long long* __restrict__ err_base) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using U = typename BucketAcc<F>::type;   // the tree runs on register-form sums (R domain): no re-packing per round
  U* sh = reinterpret_cast<U*>(smem);
  hb = item_off[hb + 1];  // the leading entries that can be heavy (msm_heavy_plan_kernel)
  const uint32_t total = item_off[hb];
  // a fixed-size grid strides over the segments: dispatching one (mostly empty) workgroup per POSSIBLE segment
  // costs milliseconds at 2^26 points
  for (uint32_t item = blockIdx.x; item < total; item += gridDim.x) {
    // bucket of this segment: last i with item_off[i] <= item
    uint32_t lo = 0, hi = hb;
    while (hi - lo > 1) {
      uint32_t mid = (lo + hi) >> 1;
      if (item_off[mid] <= item) lo = mid;
      else hi = mid;
    }
    const uint32_t b = order[lo];
    const uint32_t j0 = first[b] + (item - item_off[lo]) * seg;
    const uint32_t e = j0 + seg < last[b] ? j0 + seg : last[b];
    U a = U::zero();
    if (j0 + threadIdx.x < e)   // an R-domain record (curveu.hpp) is what every consumer of bucket sums works on: its register form here
      a = xyzzr_load(xyzzu_to_r(accumulate_run<F, false, true>(U::zero(), bases, vals, j0 + threadIdx.x, e, blockDim.x, skip_zero != 0, err_base)));
    a = wave_sum_quads(a, sh);   // (round 4: the 6-level tree on quad additions)
    if (threadIdx.x == 0) store_vec(seg_sums + item, xyzzr_store(a));
    __syncthreads();
  }
}

// bucket = sum of its segment sums (one workgroup per heavy bucket)
template <class F>
__global__ void __launch_bounds__(64) msm_heavy_combine_kernel(const XYZZ<F>* __restrict__ seg_sums, const uint32_t* __restrict__ order,
                                                              const uint32_t* __restrict__ item_off, uint32_t hb, XYZZ<F>* __restrict__ buckets,
                                                              int carry) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using U = typename BucketAcc<F>::type;
  U* sh = reinterpret_cast<U*>(smem);
  hb = item_off[hb + 1];  // the leading entries that can be heavy (msm_heavy_plan_kernel)
  for (uint32_t i = blockIdx.x; i < hb; i += gridDim.x) {
    const uint32_t lo = item_off[i], hi = item_off[i + 1];
    if (hi == lo) continue;  // not heavy (uniform per workgroup)
    U a = U::zero();
    for (uint32_t k = lo + threadIdx.x; k < hi; k += blockDim.x) xyzzr_add(a, xyzzr_load(load_vec(seg_sums + k)));
    a = wave_sum_quads(a, sh);
    if (threadIdx.x == 0) {
      if (carry) xyzzr_add(a, xyzzr_load(load_vec(buckets + order[i])));  // the bucket's sum over the earlier chunks
      store_vec(buckets + order[i], xyzzr_store(a));
    }
    __syncthreads();
  }
}

// 4b. one lane per bucket, buckets taken in size order.  Both groups run on U-form arithmetic (curveu.hpp:
//     29-bit lazy limbs, one v_mad_u64_u32 per partial product, no carry flags).
//     CARRY: the launch continues buckets that an earlier chunk of the same (streamed) multiexp has written: a bucket without
//     entries in this chunk is left alone, the others take their record up again (xyzzu_from_r: two products).
template <class F, bool A4, bool CARRY>
__global__ void __launch_bounds__(256) msm_accumulate_kernel(const Affine<F>* __restrict__ bases, const uint32_t* __restrict__ vals,
                                                            const uint32_t* __restrict__ first, const uint32_t* __restrict__ last,
                                                            const uint32_t* __restrict__ order, uint32_t heavy, uint32_t hb, uint32_t n_buckets,
                                                            XYZZ<F>* __restrict__ buckets, int skip_zero, unsigned long long* __restrict__ err_base) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_buckets) return;
  const uint32_t b = order[i];
  const uint32_t j = first[b], e = last[b];
  if (i < hb && e - j > heavy) return;  // done by msm_accumulate_heavy_kernel
  if (j >= e) {
    if constexpr (!CARRY) store_vec(buckets + b, XYZZ<F>::zero());
    return;
  }
  typename BucketAcc<F>::type acc = BucketAcc<F>::type::zero();
  // (r6, profiles/r06_carry_cost.txt: what a carried launch costs over a fresh one is its first addition -- a full mixed addition where the
  //  fresh launch copies the point into an empty accumulator -- i.e. one addition per TOUCHED BUCKET per extra chunk; the record's load and
  //  its two products are not measurable.  Adding the record at the END by a full addition instead was 1.2 x slower per launch: ~3000
  //  instructions executed once per wave run from a cold instruction cache.)
  if constexpr (CARRY) acc = xyzzu_from_r(load_vec(buckets + b));
  store_vec(buckets + b, xyzzu_to_r(accumulate_run<F, A4, !CARRY>(acc, bases, vals, j, e, 1, skip_zero != 0, err_base)));
}
// G2 with >= 2^19 buckets: the same kernel at TWO waves per SIMD.  With the rare doubling in U-form (xyzzu2_double_affine) the Fq2 loop
// needs 262 registers -- it took 256 + 147 with the saturated-limb doubling inlined -- and at a budget of 256 the seven that do not
// fit (32 B of scratch per lane) cost less than the second wave brings.  (A kernel of its own, so that the G1 instantiation of the
// template above keeps its code.)
template <bool A4, bool CARRY>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) msm_accumulate_g2w2_kernel(
    const Affine<Fq2>* __restrict__ bases, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ first, const uint32_t* __restrict__ last,
    const uint32_t* __restrict__ order, uint32_t heavy, uint32_t hb, uint32_t n_buckets, XYZZ<Fq2>* __restrict__ buckets, int skip_zero,
    unsigned long long* __restrict__ err_base) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_buckets) return;
  const uint32_t b = order[i];
  const uint32_t j = first[b], e = last[b];
  if (i < hb && e - j > heavy) return;  // done by msm_accumulate_heavy_kernel
  if (j >= e) {
    if constexpr (!CARRY) store_vec(buckets + b, XYZZ<Fq2>::zero());
    return;
  }
  XYZZU2 acc = XYZZU2::zero();
  if constexpr (CARRY) acc = xyzzu_from_r(load_vec(buckets + b));
  store_vec(buckets + b, xyzzu_to_r(accumulate_run<Fq2, A4>(acc, bases, vals, j, e, 1, skip_zero != 0, err_base)));
}

// 4b'. G2: one PAIR of lanes per bucket (curveu.hpp: PairAcc2 / pair_add_mixed -- the even lane keeps (X, ZZ) and gathers the
//     base's x, the odd lane keeps (Y, ZZZ) and gathers y; the same products as the one-lane addition, split evenly, at half the
//     registers per lane).  Same lists, same order, same records as msm_accumulate_kernel<Fq2>: bit-identical bucket sums.
template <class F, bool A4>
__device__ __forceinline__ typename PairAccOf<F>::type accumulate_run_pair(typename PairAccOf<F>::type acc, const Affine<F>* __restrict__ bases,
                                                                           const uint32_t* __restrict__ vals, uint32_t j, uint32_t e, bool odd, bool skip_zero,
                                                                           unsigned long long* __restrict__ err_base) {
  // (accumulate_run with stride 1; both lanes of the pair walk the same list and stay together)
  uint4 q = make_uint4(0, 0, 0, 0);
  uint32_t v;
  if constexpr (A4) {
    q = *reinterpret_cast<const uint4*>(vals + j);
    v = q.x;
  } else {
    v = vals[j];
  }
  const uint32_t co = odd ? 1u : 0u;
  F p = load_vec(reinterpret_cast<const F*>(bases + (v & ~SIGN_BIT)) + co);
  for (;;) {
    const uint32_t jn = j + 1;
    const bool more = jn < e;
    uint32_t vn = 0;
    F pn = p;
    if constexpr (A4) {
      if ((jn & 3u) == 0) {
        if (more) q = *reinterpret_cast<const uint4*>(vals + jn);
      } else {
        q.x = q.y; q.y = q.z; q.z = q.w;
      }
      vn = q.x;
      if (more) pn = load_vec(reinterpret_cast<const F*>(bases + (vn & ~SIGN_BIT)) + co);
    } else if (more) {
      vn = vals[jn];
      pn = load_vec(reinterpret_cast<const F*>(bases + (vn & ~SIGN_BIT)) + co);
    }
    const uint32_t ynz = pair_dpp<PAIR_ODD>(coord_or(p));   // the all-zero record is the point at infinity: y == 0 (the odd lane's coordinate)
    if (ynz != 0) {
      acc = pair_add_mixed(acc, p, (v & SIGN_BIT) != 0, odd);
    } else if (!skip_zero && odd) {
      atomicMin(err_base, (unsigned long long)(v & ~SIGN_BIT));
    }
    if (!more) break;
    v = vn;
    p = pn;
    j = jn;
  }
  return acc;
}

template <class F, bool A4, bool CARRY>
__device__ __forceinline__ void accumulate_pair_body(const Affine<F>* __restrict__ bases, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ first,
                                                     const uint32_t* __restrict__ last, const uint32_t* __restrict__ order, uint32_t heavy, uint32_t hb,
                                                     uint32_t n_buckets, XYZZ<F>* __restrict__ buckets, int skip_zero, unsigned long long* __restrict__ err_base) {
  const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x, i = gt >> 1;
  const bool odd = (gt & 1u) != 0;
  if (i >= n_buckets) return;                          // (whole pairs leave: every test up to the loop is on i)
  const uint32_t b = order[i];
  const uint32_t j = first[b], e = last[b];
  if (i < hb && e - j > heavy) return;
  F* rec = reinterpret_cast<F*>(buckets + b);          // {x, y, zz, zzz}: this lane's coordinates are rec[odd] and rec[2 + odd]
  const uint32_t co = odd ? 1u : 0u;
  if (j >= e) {
    if constexpr (!CARRY) {
      store_vec(rec + co, F::zero());
      store_vec(rec + 2 + co, F::zero());
    }
    return;
  }
  typename PairAccOf<F>::type acc = PairAccOf<F>::type::zero();
  if constexpr (CARRY) acc = pair_from_r(load_vec(rec + co), load_vec(rec + 2 + co));
  acc = accumulate_run_pair<F, A4>(acc, bases, vals, j, e, odd, skip_zero != 0, err_base);
  F oa, oz;
  pair_to_r(acc, oa, oz);
  store_vec(rec + co, oa);
  store_vec(rec + 2 + co, oz);
}
template <bool A4, bool CARRY>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2))) msm_accumulate_pair_kernel(
    const Affine<Fq2>* __restrict__ bases, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ first, const uint32_t* __restrict__ last,
    const uint32_t* __restrict__ order, uint32_t heavy, uint32_t hb, uint32_t n_buckets, XYZZ<Fq2>* __restrict__ buckets, int skip_zero,
    unsigned long long* __restrict__ err_base) {
  accumulate_pair_body<Fq2, A4, CARRY>(bases, vals, first, last, order, heavy, hb, n_buckets, buckets, skip_zero, err_base);
}
template <bool A4, bool CARRY>
__global__ void __launch_bounds__(256) msm_accumulate_pair_g1_kernel(
    const Affine<Fq>* __restrict__ bases, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ first, const uint32_t* __restrict__ last,
    const uint32_t* __restrict__ order, uint32_t heavy, uint32_t hb, uint32_t n_buckets, XYZZ<Fq>* __restrict__ buckets, int skip_zero,
    unsigned long long* __restrict__ err_base) {
  accumulate_pair_body<Fq, A4, CARRY>(bases, vals, first, last, order, heavy, hb, n_buckets, buckets, skip_zero, err_base);
}

// 4c. SHORT calls: the launch above lasts as long as its LONGEST bucket -- a lane adds a point every ~8 us however idle the device is,
//     and among 2^18 buckets of 4 points on average some hold 14 (2^16 points: 139 us of accumulation where the additions themselves
//     are 80 us of the device's time).  Buckets longer than `split_t` (and not heavy) are therefore taken out of the lane-per-bucket
//     launch and walked by a QUAD of lanes each: lane r of the quad adds entries r, r + 4, ... (its own accumulator), the four partial
//     sums are brought to all four lanes by DPP and joined by three quad additions (curveu.hpp: xyzzr_add_quad).  A 14-entry bucket is
//     then 4 mixed additions + the join instead of 14.  The buckets are order[0 .. hb) (size order): the main kernel skips them with
//     its `heavy` test set to split_t.  First chunk / unchunked calls only (no carried record).
template <class F>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) msm_accumulate_split_kernel(
    const Affine<F>* __restrict__ bases, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ first, const uint32_t* __restrict__ last,
    const uint32_t* __restrict__ order, uint32_t split_t, uint32_t heavy, uint32_t heavy_hb, uint32_t hb, XYZZ<F>* __restrict__ buckets,
    int skip_zero, unsigned long long* __restrict__ err_base) {
  using U = typename BucketAcc<F>::type;
  const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x, i = gt >> 2, role = gt & 3u;
  if (i >= hb) return;                                 // (whole quads leave: i is the same for the four lanes)
  const uint32_t b = order[i];
  const uint32_t j = first[b], e = last[b];
  // the lane-per-bucket launch has the short ones, the segment-parallel path the heavy ones AMONG order[0 .. heavy_hb): a heavy bucket
  // past that reach (more than MSM_HEAVY_BLOCKS over-long buckets: skewed exponents) is walked here -- the main kernel skips every
  // bucket of order[0 .. max(hb, heavy_hb)) longer than split_t, so nobody else would take it
  if (e - j <= split_t || (e - j > heavy && i < heavy_hb)) return;
  U part = xyzzr_load(XYZZ<F>::zero());
  if (j + role < e) part = xyzzr_load(xyzzu_to_r(accumulate_run<F, false>(U::zero(), bases, vals, j + role, e, 4, skip_zero != 0, err_base)));
  // (split_t >= 4: every lane has at least one entry; the test above is for safety)
  const U p0 = quad_fetch<0>(part), p1 = quad_fetch<1>(part), p2 = quad_fetch<2>(part), p3 = quad_fetch<3>(part);
  const U sum = xyzzr_add_quad(xyzzr_add_quad(p0, p1, role), xyzzr_add_quad(p2, p3, role), role);
  if (role == 0) store_vec(buckets + b, xyzzr_store(sum));
}

// 5. bucket reduction  T_w = sum_{k=1..nb} k * B_k  per window, without scalar multiplications:
//    split the index x = ch*L + y:   sum_x (x+off) B[x] = sum_ch A[ch] + L * sum_ch ch * S[ch]
//    with A[ch] = sum_y (y+off) B[ch*L+y] (running sums) and S[ch] = sum_y B[ch*L+y]; the second term
//    is the same problem on the L-times shorter array S with off = 0.  Each level is one launch of
//    msm_reduce_level_kernel (a lane per chunk) plus a per-window sum of its A[]; the host applies
//    the powers of L (log2 L doublings per level) while it joins the windows.
//    The two running-sum additions share ONE inlined xyzz_add (selected operands): these kernels are
//    not hot, and a single call site keeps the gfx950 code size / compile time down (Fq2 above all).
template <class F>
__global__ void __launch_bounds__(256) msm_reduce_level_kernel(const XYZZ<F>* __restrict__ in, uint32_t count, uint32_t L, uint32_t off,
                                                              uint32_t W, XYZZ<F>* __restrict__ outA, XYZZ<F>* __restrict__ outS) {
  uint32_t chunks = (count + L - 1) / L;
  uint32_t t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= chunks * W) return;
  uint32_t w = t / chunks, ch = t % chunks;
  uint32_t lo = ch * L, hi = lo + L < count ? lo + L : count;
  const XYZZ<F>* B = in + (uint64_t)w * count;
  uint32_t steps = 2 * (hi - lo);
  // R-domain records: both running sums stay in U-form registers, a bucket is re-packed (no product) when it is loaded
  auto run = xyzzr_load(XYZZ<F>::zero()), acc = run;
  for (uint32_t it = 0; it < steps; ++it) {
    uint32_t x = hi - 1 - (it >> 1);
    // off == 1: run += B[x]; acc += run   (weights y+1)      off == 0: acc += run; run += B[x]   (weights y)
    bool do_acc = ((it & 1) != 0) == (off != 0);
    auto a = do_acc ? acc : run;
    auto b = do_acc ? run : xyzzr_load(load_vec(B + x));
    xyzzr_add(a, b);
    if (do_acc) acc = a;
    else run = a;
  }
  store_vec(outA + t, xyzzr_store(acc));
  store_vec(outS + t, xyzzr_store(run));
}

// The same level with a QUAD of lanes per chunk (curveu.hpp: xyzzr_add_quad -- four lanes share the products of every addition):
// for the levels that are left with too few chunks to fill the device, where a lane's 2L dependent additions are what the launch
// lasts.  Lanes 4t .. 4t+3 hold the same running sums.
template <class F>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) msm_reduce_level_quad_kernel(const XYZZ<F>* __restrict__ in, uint32_t count, uint32_t L, uint32_t off,
                                                                   uint32_t W, XYZZ<F>* __restrict__ outA, XYZZ<F>* __restrict__ outS) {
  const uint32_t chunks = (count + L - 1) / L;
  const uint32_t gt = blockIdx.x * blockDim.x + threadIdx.x, t = gt >> 2, role = gt & 3u;
  if (t >= chunks * W) return;   // (whole quads leave: t is the same for the four lanes)
  const uint32_t w = t / chunks, ch = t % chunks;
  const uint32_t lo = ch * L, hi = lo + L < count ? lo + L : count;
  const XYZZ<F>* B = in + (uint64_t)w * count;
  // run_x = B[x] + .. + B[hi-1];  acc = sum of run_x over x (off == 1: weights y + 1) or over x > lo (off == 0: weights y).
  // (two call sites and no selected operands: with the lane kernel's `a = do_acc ? acc : run` hipcc kept the sums in scratch here)
  auto run = xyzzr_load(XYZZ<F>::zero()), acc = run;
  for (uint32_t x = hi; x-- > lo;) {
    run = xyzzr_add_quad(run, xyzzr_load(load_vec(B + x)), role);
    if (off != 0 || x > lo) acc = xyzzr_add_quad(acc, run, role);
  }
  if (role == 0) store_vec(outA + t, xyzzr_store(acc));
  if (role == 1) store_vec(outS + t, xyzzr_store(run));
}

// 5b/5c. the tail of the reduction, by trees.  A running-sum level costs 2L dependent additions however few
//     elements are left, so once at most MSM_FINAL_MAX elements per window remain the weighted sum of the last S[]
//     is finished by BIT DECOMPOSITION:  sum_x (x+off) S[x] = sum_j 2^j * (sum over x with bit j of (x+off) set of S[x]),
//     and the plain sums of every level's A[] ride in the same launch.  One workgroup sums a slice of MSM_TREE_SLICE
//     elements of one job (A of a level, or one bit) of one window: one pair per lane, then an LDS tree (depth 9);
//     further launches of the same kernel sum the slice sums.  The host applies the powers of two and of L.
//     The grid is 1-D over the NON-EMPTY (window, job, slice) triples: jobs of one launch differ in length, and a
//     (slices, jobs, windows) grid put every short job's only workgroup on the same XCD (block id = multiple of 8).
template <class F>
struct TreeJobs {
  // job j sums the elements x < cnt[j] of  in[j] + w * stride[j] + rep * rep_stride[j]  taken elem_stride[j] apart (bit[j] < 0), or
  // only the x with bit bit[j] of (x + off[j]) set; a job is a FAMILY of reps[j] such sums (the rows / the columns of the 2-D tail);
  // an element exists while rep * rep_stride + x * elem_stride < limit[j]
  const XYZZ<F>* in[MSM_MAX_JOBS];
  XYZZ<F>* out[MSM_MAX_JOBS];        // slice sum of (w, rep, slice) -> out[j][(w * out_w[j] + rep) * slices(j) + slice]
  uint32_t cnt[MSM_MAX_JOBS];
  uint32_t stride[MSM_MAX_JOBS];
  uint32_t reps[MSM_MAX_JOBS], rep_stride[MSM_MAX_JOBS], elem_stride[MSM_MAX_JOBS], limit[MSM_MAX_JOBS];
  uint32_t out_w[MSM_MAX_JOBS];
  uint32_t off[MSM_MAX_JOBS];
  int32_t bit[MSM_MAX_JOBS];
  uint32_t first_block[MSM_MAX_JOBS + 1];  // prefix sums of reps * slices: blocks per window = first_block[n_jobs]
  uint32_t n_jobs;
  uint32_t quad;                           // 1: the last rounds of a slice's tree run four lanes per addition (G1)
};
template <class F>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) msm_tree_kernel(const TreeJobs<F> J) {
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  using U = typename BucketAcc<F>::type;   // sums travel between the rounds in REGISTER form (U-form limbs): no re-packing per round
  U* sh = reinterpret_cast<U*>(smem);
  const uint32_t per_w = J.first_block[J.n_jobs];
  const uint32_t w = blockIdx.x / per_w, r = blockIdx.x % per_w;
  uint32_t job = 0;
  while (job + 1 < J.n_jobs && J.first_block[job + 1] <= r) ++job;
  const uint32_t count = J.cnt[job];
  const uint32_t slices = (count + MSM_TREE_SLICE - 1) / MSM_TREE_SLICE;
  const uint32_t idx = r - J.first_block[job];
  const uint32_t rp = idx / slices, slice = idx % slices;
  const int32_t bit = J.bit[job];
  const uint32_t off = J.off[job], es = J.elem_stride[job];
  const uint32_t rbase = rp * J.rep_stride[job], limit = J.limit[job];
  const XYZZ<F>* P = J.in[job] + (uint64_t)w * J.stride[job] + rbase;
  const uint32_t x0 = slice * MSM_TREE_SLICE + threadIdx.x, x1 = x0 + 256;
  XYZZ<F> r0 = XYZZ<F>::zero(), r1 = XYZZ<F>::zero();
  if (x0 < count && (uint64_t)rbase + (uint64_t)x0 * es < limit && (bit < 0 || (((x0 + off) >> bit) & 1))) r0 = load_vec(P + (uint64_t)x0 * es);
  if (x1 < count && (uint64_t)rbase + (uint64_t)x1 * es < limit && (bit < 0 || (((x1 + off) >> bit) & 1))) r1 = load_vec(P + (uint64_t)x1 * es);
  U acc = xyzzr_load(r0), other = xyzzr_load(r1);   // (the zero record loads as the zero accumulator: ZZ == 0 limbs)
  // ONE inlined xyzz_add for the pair and for every tree level (code size).  Lanes [s, 2s) publish, lanes [0, s)
  // consume; the regions written in consecutive rounds are disjoint from the ones still being read, so one
  // barrier per round.
  // Round 4: once at most 64 additions are left in a round, FOUR lanes share each of them (curveu.hpp: xyzzr_add_quad): the
  // last seven rounds are a chain of seven additions on an otherwise idle workgroup, and a quad's addition is three products +
  // one double product deep instead of fourteen.  J.quad == 0 keeps the one-lane rounds (the comparison).
  const uint32_t quad_from = J.quad ? 128u : 0u;   // the value of s after which the quads take over
  for (uint32_t s = 256;;) {
    xyzzr_add(acc, other);   // (its results keep the invariants its operands need: the running-sum levels chain it the same way)
    s >>= 1;
    if (s == 0 || s < quad_from) break;
    if (threadIdx.x >= s && threadIdx.x < 2 * s) sh[threadIdx.x] = acc;
    __syncthreads();
    other = threadIdx.x < s ? sh[threadIdx.x + s] : U::zero();
  }
  {
    if (quad_from) {
      // lanes 0 .. 127 hold the sums of the round s = 128; quad q = lane / 4 continues element q
      if (threadIdx.x < 128) sh[threadIdx.x] = acc;
      __syncthreads();
      const uint32_t q = threadIdx.x >> 2, role = threadIdx.x & 3u;
      acc = sh[q];
      for (uint32_t s = 64; s > 0; s >>= 1) {
        if (q < s) {                       // (uniform over a quad)
          acc = xyzzr_add_quad(acc, sh[q + s], role);
          if (role == 0) sh[q] = acc;      // read by quad q - s/2 in the next round (when q >= s/2)
        }
        __syncthreads();
      }
    }
  }
  if (threadIdx.x == 0) store_vec(J.out[job] + ((uint64_t)w * J.out_w[job] + rp) * slices + slice, xyzzr_store(acc));
}

// Table mode, error path only: the accumulation reports the lowest TABLE index that held the identity, which orders by window
// first; the reference reports the lowest EXPONENT (source.rs:50-52).  One pass over the exponents and their bases (the table's first
// window) finds it: the lowest base index that is the identity under a selected, non-zero exponent.
template <class F>
__global__ void __launch_bounds__(256) msm_identity_scan_kernel(const Affine<F>* __restrict__ bases, const uint32_t* __restrict__ scalars, uint64_t n,
                                                               uint64_t base_offset, const uint32_t* __restrict__ density,
                                                               const uint32_t* __restrict__ dprefix, unsigned long long* __restrict__ err_base) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint64_t bi = base_offset + i;
  if (density != nullptr) {
    const uint32_t wd = density[i >> 5];
    if (!((wd >> (i & 31)) & 1u)) return;
    bi = base_offset + dprefix[i >> 5] + __popc(wd & ((1u << (i & 31)) - 1u));
  }
  const uint4* sp = reinterpret_cast<const uint4*>(scalars + i * 8);
  const uint4 s0 = sp[0], s1 = sp[1];
  if ((s0.x | s0.y | s0.z | s0.w | s1.x | s1.y | s1.z | s1.w) == 0) return;
  if (load_affine(bases + bi).y.is_zero()) atomicMin(err_base, (unsigned long long)bi);
}

// ------------------------------------------------------------------------------------------------
// Segmented sum of affine points (msm_host.hpp: segsum_device): the index list of the identity order, and the normalisation of the row sums.
__global__ void __launch_bounds__(256) msm_iota_kernel(uint32_t* __restrict__ v, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = i;
}
template <class F>
__global__ void __launch_bounds__(256) msm_to_affine_kernel(const XYZZ<F>* __restrict__ in, Affine<F>* __restrict__ out, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = xyzz_to_affine(load_vec(in + i));
}

}  // namespace

}  // namespace zk
