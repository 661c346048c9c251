// Radix-2 number-theoretic transform over BN254 Fr for gfx950 (MI355X).
//
// Replaces, behind the C ABI of include/mi355zk.h, the reference's
//   bellman/src/domain.rs:263-376  best_fft / serial_fft / parallel_fft   (-> ntt_run)
//   bellman/src/domain.rs:159-203  ifft scaling, distribute_powers, coset_fft, icoset_fft (fused in)
// for `Scalar<Bn256>` elements (bellman/src/group.rs:53-82): 32-byte Montgomery Fr limbs, natural
// order in, natural order out, in place.
//
// Algorithm (not the reference's): a size-N transform is factored N = N_1 * ... * N_R (R <= 3,
// N_p <= 4096, normally 1024) Cooley-Tukey style.  Pass p transforms digit p of the index for G adjacent
// "columns" at once: a workgroup stages a G x N_p tile (<= 4096 elements) in LDS on nine 29-bit limbs per
// element (U-form, fieldu.hpp; element-major, see lds_load), runs log2(N_p) DIT stages
// there, multiplies by the inter-pass twiddle omega^(T_p*k_p*rest) and writes back in the 32-byte
// memory format.  The last pass writes straight to the natural-order position (fused digit reversal),
// with the G tile rows chosen so that both its loads and its stores are >= 128-byte contiguous.
// distribute_powers (coset) is fused into the first pass's load, the 1/m and g^-k scalings into the
// last pass's store.  HBM traffic: 64 B per element per pass (R passes) -- DESIGN.md "NTT".
//
// U-form bookkeeping (fieldu.hpp): data stays in the memory format's 2^256 domain the whole time -- every
// product is by a table twiddle, kept as the PLAIN integer w with its quotient floor(w 2^261 / p), and
// the Shoup product of fieldu.hpp returns data*w itself, below 2p (round 4; rounds 1-3: Montgomery products by
// twiddles in the 2^261 domain, 180 multiplier instructions against 143) -- so loads and stores only
// re-pack bits.  DIT butterflies (a + w b, a - w b) grow values linearly: V_s <= V_0 + 2 s p <= 22p after
// 10 stages without a skipped product, 30p with the skipped twiddle-one products (values double there), far below
// the 160p the product admits and below the 32p of the closing reduction; limbs are carried every 4th stage.  The
// arithmetic and its bounds are stated once, in ntt_butterfly.hpp, and derived by tests/cpp/test_ntt_bounds_host.cpp.
// The mathematical result X[k] = sum_i a[i] w^(ik) is unique and the stored elements are fully
// reduced, so the output bytes are identical to serial_fft's.
#define ZK_CHAIN_MAD 1  // fieldu.hpp u_mad: one dependent mad chain per column (measured faster in this TU)
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "fieldu.hpp"
#include "ntt_butterfly.hpp"  // TwU, tw_mul, tw_make; NttSchedule, ntt_bf and every other line of field arithmetic a pass runs
#include "device_util.hpp"
#include "ntt_plan.hpp"  // NttPassParams, NttBatch, the NTT_* constants; NttKnobs and the planner

namespace zk {

namespace {

// table entry (round 4): a twiddle as the PLAIN canonical integer w on nine 29-bit limbs followed by wq = floor(w * 2^261 / p) --
// the constant and its quotient of fieldu.hpp's u_mul_shoup -- 72 B, 8-byte aligned (padding the entry to 80 B for aligned 16-byte
// loads measured 0.5-1 % slower: tools/ab_ntt_shoup.sh).  (Rounds 1-3: w * 2^261 mod p for the Montgomery product, 48 B.)
struct alignas(8) UTab {
  uint32_t l[18];
};
__device__ __forceinline__ TwU tab_load(const UTab* p) {
  const uint2* s = reinterpret_cast<const uint2*>(p);   // (hipcc merges neighbours into 16-byte loads where the address allows)
  uint32_t v[18];
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    const uint2 t = s[i];
    v[2 * i] = t.x;
    v[2 * i + 1] = t.y;
  }
  TwU r;
#pragma unroll
  for (int i = 0; i < 9; ++i) { r.w.l[i] = v[i]; r.q.l[i] = v[9 + i]; }
  return r;
}
__device__ __forceinline__ void tab_store(UTab* p, const TwU& t) {
  UTab e;
#pragma unroll
  for (int i = 0; i < 9; ++i) { e.l[i] = t.w.l[i]; e.l[9 + i] = t.q.l[i]; }
  *p = e;
}

// LDS layout of a tile (round 4): ELEMENT-major, nine consecutive words per element.  The stride of 9 words is odd, so lanes with
// consecutive (or swz-permuted) element indices still sit on different banks -- bank = (9 idx + l) mod 32 is idx mod 32 up to a
// bijection -- and the nine limbs of an element are at FIXED offsets from ONE address: ds_read / ds_write take them as immediates
// (hipcc pairs them into ds_read2_b32), where the limb-PLANE layout of rounds 1-3 (lds[l * plane + idx], plane a run-time value)
// cost one VALU add and one address register per limb: 36 address registers per radix-4 group, ~85 VALU instructions per
// element and pass.  -DZK_NTT_LDS_PLANES restores the planes for the comparison.
__device__ __forceinline__ FrU lds_load(const uint32_t* lds, uint32_t plane, uint32_t idx) {
  FrU r;
#ifdef ZK_NTT_LDS_PLANES
#pragma unroll
  for (int l = 0; l < 9; ++l) r.l[l] = lds[l * plane + idx];
#else
  (void)plane;
  const uint32_t* e = lds + idx * 9u;
#pragma unroll
  for (int l = 0; l < 9; ++l) r.l[l] = e[l];
#endif
  return r;
}
__device__ __forceinline__ void lds_store(uint32_t* lds, uint32_t plane, uint32_t idx, const FrU& v) {
#ifdef ZK_NTT_LDS_PLANES
#pragma unroll
  for (int l = 0; l < 9; ++l) lds[l * plane + idx] = v.l[l];
#else
  (void)plane;
  uint32_t* e = lds + idx * 9u;
#pragma unroll
  for (int l = 0; l < 9; ++l) e[l] = v.l[l];
#endif
}
__device__ __forceinline__ Fr gload(const Fr* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint4 a = q[0], b = q[1];
  Fr r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  return r;
}
__device__ __forceinline__ void gstore(Fr* p, const Fr& v) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

__device__ __forceinline__ uint32_t bitrev(uint32_t x, uint32_t bits) { return bits ? (__brev(x) >> (32 - bits)) : 0; }

// Row-local LDS position of element x: the low five bits (the bank, up to the odd element stride 9) are XOR-ed with a mix of the bits
// above them.  Round 4 XOR-ed bits 5..9 in unchanged and padded the rows to np + 1 elements: tools/ntt_lds_model.py (a bank model of every
// access site of this kernel; it reproduces the counter) showed where its 20 % conflict cycles on the 2^20 pass came from -- the stage pair
// with m = 16 (lanes 16 apart hold x and x + 64, and "+ 64" moved the position by 2, inside the same 16 banks) and the closing read of a
// G >= 2 tile (neighbouring lanes alternate rows at +9 banks per row against +9 per element) -- and 33 - 58 % on the tiles of 2^21 .. 2^26.
// Now: bits 5..9 times 25 (so that x + 32, + 64, + 128 ... each land in another part of the 32 banks), bits 10, 11 of the long rows folded
// in, rows at the plain pitch np and told apart by a row term (lds_pos).  Modelled conflict cycles: 2^20 pass 20 % -> 0, 2^21 .. 2^23
// 26 - 33 % -> 0, 2^24 58 % -> 20 %, 2^25 / 2^26 45 % -> 1 %; measured: profiles/r05_ntt20_pass_sq_pmc.txt.
__device__ __forceinline__ uint32_t swz(uint32_t x) { return x ^ ((((x >> 5) * 25u) ^ (x >> 10)) & 31u); }
// position of element x of row g in a tile of rows of np >= 32 elements: `rowx` = (g * a) & 31 with a = 21 (a = 20 for eight-row tiles)
// moves neighbouring rows to other banks where lanes alternate rows (tile load and store); shorter rows are not permuted (swz is the identity there)
__device__ __forceinline__ uint32_t row_term(uint32_t g, uint32_t G, uint32_t np) { return np >= 32 ? (g * (G == 8 ? 20u : 21u)) & 31u : 0u; }

// One pass over one tile.  roots[x] = w_p^x for x < N_p/2 (w_p = omega^(N/N_p)).
template <uint32_t LOG_NP, bool R4>
__global__ void __launch_bounds__(NTT_THREADS) ntt_pass_kernel(const Fr* __restrict__ in, Fr* __restrict__ out, NttPassParams P,
                                                              const UTab* __restrict__ roots, const UTab* __restrict__ twA,
                                                              const UTab* __restrict__ twB, const UTab* __restrict__ preA,
                                                              const UTab* __restrict__ preB, const UTab* __restrict__ postA,
                                                              const UTab* __restrict__ postB, TwU post_c, const UTab* __restrict__ twF, NttBatch BP) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  constexpr uint32_t np = 1u << LOG_NP;
  // twiddle-one products are skipped in the stages the schedule allows (ntt_butterfly.hpp: rows longer than 2^10 give up stage 2)
  using SCH = NttSchedule<LOG_NP>;
  constexpr uint32_t pitch = np;
  const uint32_t plane = P.g * pitch;
  const uint32_t elems = P.g * np;
  // One- and two-row tiles move 32- / 64-byte runs at a large stride: a fraction of every DRAM burst and page, the rest belonging to
  // the neighbouring tiles.  Workgroup ids go round the eight XCDs, so neighbours would sit behind different L2s; instead the 32 tiles
  // an XCD runs at a time (ids b + 8k) are made NEIGHBOURS, so that the XCD's L2 sees kilobyte runs.
  uint64_t tile = blockIdx.x;
  if (P.batch > 1) {                                   // (uniform: scalar loads of the transform's two pointers from the kernel arguments)
    const uint32_t bt = (uint32_t)(tile / P.tiles);
    tile -= (uint64_t)bt * P.tiles;
    in = BP.in[bt];
    out = BP.out[bt];
  }
  if (P.xcd_pair == 1) tile = (tile & ~15ull) | ((tile & 7ull) << 1) | ((tile >> 3) & 1ull);
  else if (P.xcd_pair == 5) tile = (tile & ~255ull) | ((tile & 7ull) << 5) | ((tile >> 3) & 31ull);  // 32 neighbours per XCD: what it runs at a time
  const uint64_t hi = tile / P.tiles_lo, lo = tile % P.tiles_lo;
  const uint64_t in_base = hi * P.in_hi_stride + lo * P.in_lo_stride;
  const uint64_t out_base = hi * P.out_hi_stride + lo * P.out_lo_stride;

  // load (bit-reversed placement inside each row: the DIT stages below then finish in natural order)
  for (uint32_t e = threadIdx.x; e < elems; e += blockDim.x) {
    uint32_t x, g;
    if (P.load_x_fastest) { x = e & (np - 1); g = e >> LOG_NP; }
    else { g = e % P.g; x = e / P.g; }
    const uint64_t gi = in_base + x * P.in_xs + g * P.in_gs;
    FrU v = ntt_load(gload(in + gi));                                     // < p, N
    if (P.pre == 1) {                                                     // distribute_powers (domain.rs:176-189)
      v = ntt_pre1(v, tab_load(preA + (gi >> P.pre_h)), [&] { return tab_load(preB + (gi & ((1ull << P.pre_h) - 1))); });   // g^i = A[i >> h] * B[i & mask]: < 2p, N
    } else if (P.pre == 2) {
      v = ntt_pre2(v, tab_load(preA + x));                                // (g^S)^x: the column's g^col sits in the folded inter-pass table
    }
    lds_store(lds, plane, g * pitch + (swz(bitrev(x, LOG_NP)) ^ row_term(g, P.g, np)), v);
  }
  __syncthreads();

  // DIT stages.  Entering stage s every element has limbs < ((s & 3) + 1) * 2^29 and is < (4 + 2s) p, or < 16p + 2(s - 3)p when
  // the twiddle-one products of stages 1 and 2 are skipped (see j_slow): the chain is stated in ntt_butterfly.hpp and derived, stage by
  // stage, by the host bound checker (tests/cpp/test_ntt_bounds_host.cpp).
  if constexpr (R4) {
  // (LOG_NP is a template parameter and the stage loops are static: the stage number, the skip / carry decisions and the shift amounts
  // of the index arithmetic are compile-time constants in every stage)
  // One butterfly of stage ST on registers (ntt_bf): (u, t) -> (u + w t, u - w t); skip: w = 1 (stage 0; twiddle index 0 of stages 1 and 2).
  const auto bf = ntt_bf_fn<SCH>();
  constexpr uint32_t S0 = LOG_NP & 1;  // an odd number of stages: stage 0 alone (all twiddles one), then pairs
  if constexpr (S0 == 1) {
    const uint32_t half = elems >> 1;
    for (uint32_t b = threadIdx.x; b < half; b += blockDim.x) {
      const uint32_t g = b >> (LOG_NP - 1), x0 = (b & ((np >> 1) - 1)) << 1;
      const uint32_t rx = row_term(g, P.g, np);
      const uint32_t i0 = g * pitch + (swz(x0) ^ rx), i1 = g * pitch + (swz(x0 + 1) ^ rx);
      FrU u = lds_load(lds, plane, i0), t = lds_load(lds, plane, i1);
      bf(std::integral_constant<int, 0>{}, u, t, TwU{u, u}, true);
      lds_store(lds, plane, i0, u);
      lds_store(lds, plane, i1, t);
    }
    __syncthreads();
  }
  // Two stages per LDS round trip: a lane holds the four elements x0 + {0, m, 2m, 3m} (m = 2^s), runs the two butterflies of stage s
  // (same twiddle w^j) and the two of stage s + 1 (twiddle indices j and j + m) on registers.  For the pair that starts at stage 1
  // or 2 the groups of a row are dealt to the lanes with the twiddle index j SLOWEST (lane = j * blocks + block), so j is uniform
  // over a wave and the waves with j == 0 -- twiddle one -- skip those products; later pairs: j fastest (unit-stride LDS).
  const uint32_t quarter = elems >> 2;
  for_limbs<(int)(LOG_NP / 2)>([&](auto pc) {
    constexpr uint32_t s = S0 + 2u * (uint32_t) decltype(pc)::value;
    constexpr uint32_t m = 1u << s;
    constexpr bool j_slow = (s == 1 || s == 2) && (np >> (s + 2)) >= 64;
    for (uint32_t q = threadIdx.x; q < quarter; q += blockDim.x) {
      const uint32_t g = q >> (LOG_NP - 2);
      const uint32_t qf = q & ((np >> 2) - 1);
      uint32_t j, x0;
      if constexpr (j_slow) {
        constexpr uint32_t blocks_log = LOG_NP - 2 - s;                    // blocks of 4m per row
        j = qf >> blocks_log;
        x0 = ((qf & ((1u << blocks_log) - 1u)) << (s + 2)) + j;
      } else {
        j = qf & (m - 1);
        x0 = ((qf >> s) << (s + 2)) + j;
      }
      const uint32_t row = g * pitch, rx = row_term(g, P.g, np);
      const uint32_t ia = row + (swz(x0) ^ rx), ib = row + (swz(x0 + m) ^ rx), ic = row + (swz(x0 + 2 * m) ^ rx), id = row + (swz(x0 + 3 * m) ^ rx);
      FrU a = lds_load(lds, plane, ia), b = lds_load(lds, plane, ib), c = lds_load(lds, plane, ic), d = lds_load(lds, plane, id);
      const bool one = SCH::may_skip(s) && j == 0;                            // stage s (s == 0: j == 0 always)
      {
        TwU w1{a, a};
        if (!one) w1 = tab_load(roots + ((uint64_t)j << (LOG_NP - 1 - s)));
        bf(std::integral_constant<int, (int)s>{}, a, b, w1, one);
        bf(std::integral_constant<int, (int)s>{}, c, d, w1, one);
      }
      const bool one2 = SCH::may_skip(s + 1) && j == 0;                       // stage s + 1, pair (a, c): index j
      {
        TwU w2{a, a};
        if (!one2) w2 = tab_load(roots + ((uint64_t)j << (LOG_NP - 2 - s)));
        bf(std::integral_constant<int, (int)s + 1>{}, a, c, w2, one2);
      }
      {
        const TwU w3 = tab_load(roots + ((uint64_t)(j + m) << (LOG_NP - 2 - s)));   // pair (b, d): index j + m, never zero
        bf(std::integral_constant<int, (int)s + 1>{}, b, d, w3, false);
      }
      lds_store(lds, plane, ia, a);
      lds_store(lds, plane, ib, b);
      lds_store(lds, plane, ic, c);
      lds_store(lds, plane, id, d);
    }
    __syncthreads();
  });
  } else {
  // radix-2 stages (short transforms run narrow tiles, at least 256 of them: a pass is latency-bound there, and two independent
  // butterflies per lane and stage beat one group of four on half the lanes: 2^16 0.048 ms against 0.053)
  const uint32_t half = elems >> 1;
  // (LOG_NP is a template parameter and the stage loop a static one: the stage number, the skip / carry decisions and the shift
  // amounts of the index arithmetic are compile-time constants in every stage)
  for_limbs<(int)LOG_NP>([&](auto sc) {
    constexpr uint32_t s = (uint32_t) decltype(sc)::value;
    constexpr uint32_t m = 1u << s;
    // Stages 1 and 2 (when a row has at least 64 blocks of 2m): the butterflies of a row are dealt to the lanes with the
    // twiddle index j SLOWEST (lane = j * blocks + block), so j is uniform over a wave and the waves with j == 0 -- twiddle
    // one: 1/2 and 1/4 of the butterflies of these stages -- skip the product.  Later stages: j fastest (unit-stride LDS).
    // (Bounds: ntt_butterfly.hpp.)
    constexpr bool j_slow = s >= 1 && SCH::may_skip(s) && (np >> (s + 1)) >= 64;
    for (uint32_t b = threadIdx.x; b < half; b += blockDim.x) {
      uint32_t g = b >> (LOG_NP - 1);
      uint32_t bf = b & ((np >> 1) - 1);
      uint32_t j, x0;
      if (j_slow) {
        const uint32_t blocks_log = LOG_NP - 1 - s;                     // blocks of 2m per row
        j = bf >> blocks_log;
        x0 = ((bf & ((1u << blocks_log) - 1u)) << (s + 1)) + j;
      } else {
        j = bf & (m - 1);
        x0 = ((bf >> s) << (s + 1)) + j;
      }
      const uint32_t rx = row_term(g, P.g, np);
      uint32_t i0 = g * pitch + (swz(x0) ^ rx);
      uint32_t i1 = g * pitch + (swz(x0 + m) ^ rx);
      FrU u = lds_load(lds, plane, i0);
      FrU t = lds_load(lds, plane, i1);
      const bool skip = (s == 0) || (j_slow && j == 0);                   // w = 1 (stage 0; j == 0): no product
      FrU sum, dif;
      const UTab* const tw = roots + ((uint64_t)j << (LOG_NP - 1 - s));
      ntt_bf_to<s, SCH>(u, t, [&]() __attribute__((always_inline)) { return tab_load(tw); }, skip, sum, dif);
      lds_store(lds, plane, i0, sum);
      lds_store(lds, plane, i1, dif);
    }
    __syncthreads();
  });
  }

  // store: one more product brings the value below 2p (inter-pass twiddle, or the post scale / one on the last pass)
  for (uint32_t e = threadIdx.x; e < elems; e += blockDim.x) {
    uint32_t g = e % P.g, k = e / P.g;
    FrU v = lds_load(lds, plane, g * pitch + (swz(k) ^ row_term(g, P.g, np)));   // < 30p, limbs < 4*2^29
    const uint64_t go = out_base + k * P.out_xs + g * P.out_gs;
    TwU w;
    if (P.tw_full) {
      w = tab_load(twF + go);                                             // w^(k * col), streamed: one product instead of two
    } else if (P.tw_mul != 0) {
      uint64_t ex = P.tw_mul * k * (lo * P.g + g);
      v = ntt_post_mul(v, tab_load(twA + (ex >> P.tw_h)));                // w^ex = A[ex >> h] * B[ex & mask]
      w = tab_load(twB + (ex & ((1ull << P.tw_h) - 1)));
    } else if (P.post == 2) {                                             // minv * ginv^k (icoset_fft, domain.rs:197-203)
      v = ntt_post_mul2(v, tab_load(postA + (go >> P.post_h)), [&] { return tab_load(postB + (go & ((1ull << P.post_h) - 1))); });
      w = post_c;
    } else if (P.post == 3) {                                             // plain fft / coset_fft: nothing to multiply by --
      gstore(out + go, ntt_store_plain(v));                               // reduce the < 30p value directly
      continue;
    } else if (P.post == 4) {
      w = tab_load(postA + k);                                            // (ginv^N1)^k; minv * ginv^k1 sits in the folded inter-pass table
    } else {
      w = post_c;                                                         // minv (ifft, domain.rs:163-173)
    }
    const FrU prod = ntt_post_mul(v, w);                                   // v < 30p, limbs < 4*2^29: < 2p
    gstore(out + go, ntt_reduce_lt2p(prod));
  }
}

// ------------------------------------------------------------------------------------------------
// Round 5: the radix-4 pass with WAVE-LOCAL stage pairs (full tiles: G * np = 2048 or 4096 elements, a lane per group of four).
// Same arithmetic per element as ntt_pass_kernel<LOG_NP, true> above (same butterflies, same skipped twiddle-one products, hence the
// same value bounds and the same bytes); what changes is WHICH lane runs which group and how the lanes wait for one another:
//   * lane q takes row g = q mod G and group index qf = q / G in EVERY stage pair (twiddle index j = qf mod m fastest).  A wave
//     therefore owns 64 / G consecutive groups of every row, i.e. an aligned block of 256 / G elements per row, for as long as the
//     groups of a stage pair span no more than that block: the hand-over from pair s to pair s + 2 then stays inside the wave -- the
//     LDS executes a wave's writes and reads in order -- and needs NO workgroup barrier.  For the 2 x 1024 tiles of a 2^20 transform
//     that removes the barriers behind pairs 0 and 2; with the two below, 2 barriers are left of 6.  (Measured before the rewrite, by
//     deleting those barriers from the old kernel -- wrong results, right cost: 61.0 -> 58.6 us per pass.)
//   * column passes load every lane's first group straight into registers: the elements of a group of pair 0 sit at bit-reversed
//     positions 4 qf + k, i.e. they are the elements brev(k) * np / 4 + brev(qf) of the row -- rows of a column pass are strided in
//     memory anyway, so these loads coalesce exactly like the old tile load (G adjacent 32-byte records per element index) -- and
//     the tile's first LDS round trip and the barrier behind the load disappear.  The last pass (rows contiguous in memory) keeps
//     the coalesced tile load through LDS.
//   * the last stage pair leaves the lane with the elements j + r * np / 4 of its row in natural order: they are multiplied by the
//     inter-pass twiddle / scale and stored from registers (G adjacent records per element index, as before): no closing LDS round
//     trip and barrier either.
// The twiddle-one skip of the old kernel's pair 1 / 2 relied on dealing the groups j-slowest; here a lane whose j is 0 still takes
// the skipping branch (same arithmetic), its wave just does not save the time.
// LDS positions: swizzle multiplier 13 and per-G row terms chosen with the bank model for THIS lane order (tools/ntt_lds_model.py).
__device__ __forceinline__ uint32_t swz_wl(uint32_t x) { return x ^ ((((x >> 5) * 13u) ^ (x >> 10)) & 31u); }
__device__ __forceinline__ uint32_t row_term_wl(uint32_t g, uint32_t G) { return (g * (G == 2 ? 26u : G == 4 ? 21u : 25u)) & 31u; }
__device__ __forceinline__ void wave_handover() {
  // the wave's LDS writes of this stage pair before its reads of the next: nothing for the hardware (in order per wave), an order for the compiler
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <uint32_t LOG_NP>
__global__ void __launch_bounds__(NTT_THREADS) ntt_pass_wl_kernel(const Fr* __restrict__ in, Fr* __restrict__ out, NttPassParams P,
                                                                 const UTab* __restrict__ roots, const UTab* __restrict__ twA,
                                                                 const UTab* __restrict__ twB, const UTab* __restrict__ preA,
                                                                 const UTab* __restrict__ preB, const UTab* __restrict__ postA,
                                                                 const UTab* __restrict__ postB, TwU post_c, const UTab* __restrict__ twF, NttBatch BP) {
  extern __shared__ __attribute__((aligned(16))) uint32_t lds[];
  static_assert(LOG_NP >= 8, "full tiles of rows of at least 256 elements");
  constexpr uint32_t np = 1u << LOG_NP;
  using SCH = NttSchedule<LOG_NP>;                      // as in ntt_pass_kernel
  constexpr uint32_t pitch = np;
  constexpr uint32_t plane = 0;                         // (element-major tiles only)
  const uint32_t G = P.g, log_g = 31u - (uint32_t)__clz(G);
  const uint32_t elems = G * np;                        // == 4 * blockDim.x
  uint64_t tile = blockIdx.x;
  if (P.batch > 1) {
    const uint32_t bt = (uint32_t)(tile / P.tiles);
    tile -= (uint64_t)bt * P.tiles;
    in = BP.in[bt];
    out = BP.out[bt];
  }
  if (P.xcd_pair == 1) tile = (tile & ~15ull) | ((tile & 7ull) << 1) | ((tile >> 3) & 1ull);
  else if (P.xcd_pair == 5) tile = (tile & ~255ull) | ((tile & 7ull) << 5) | ((tile >> 3) & 31ull);
  const uint64_t hi = tile / P.tiles_lo, lo = tile % P.tiles_lo;
  const uint64_t in_base = hi * P.in_hi_stride + lo * P.in_lo_stride;
  const uint64_t out_base = hi * P.out_hi_stride + lo * P.out_lo_stride;
  const uint32_t q = threadIdx.x;
  // (a wave whose lanes share ONE row would own 256 elements of it and need one barrier less -- but its loads and stores are then lone
  // 32-byte records, the neighbour column's record going to another wave: measured 0.117 -> 0.139 ms at 2^20, 1.96 -> 2.66 ms at 2^24)
  const uint32_t g = q & (G - 1u), qf = q >> log_g;    // row, group index (qf < np / 4)
  const uint32_t own = 256u / G;                        // elements of a row a wave owns
  const uint32_t row = g * pitch, rx = row_term_wl(g, G);
  // P.pre == 3 (folded tables): the row twist of a coset transform sits in the butterfly twiddles -- a stage-major table (ntt_stage_table_kernel)
  // in preA instead of `roots`, and no twiddle is one
  const bool twisted = P.pre >= 3;
  const UTab* stage_tab = twisted ? preA : roots;
  auto at = [&](uint32_t x) __attribute__((always_inline)) { return row + (swz_wl(x) ^ rx); };

  auto fetch = [&](uint64_t gi, uint32_t x) __attribute__((always_inline)) {           // element x of a row from memory: < 2p, N
    FrU v = ntt_load(gload(in + gi));
    if (P.pre == 4) v = ntt_pre4(v, tab_load(preB + (gi - (uint64_t)x * P.in_xs)));   // transforms without a full table: g^col (a first pass: gi = x * S + col)
    if (P.pre == 1) {                                   // distribute_powers (domain.rs:176-189)
      v = ntt_pre1(v, tab_load(preA + (gi >> P.pre_h)), [&] { return tab_load(preB + (gi & ((1ull << P.pre_h) - 1))); });
    } else if (P.pre == 2) {
      v = ntt_pre2(v, tab_load(preA + x));              // folded tables: (g^S)^x here, g^col in the inter-pass table
    }
    return v;
  };
  // (the butterfly of ntt_pass_kernel: ntt_bf)
  const auto bf = ntt_bf_fn<SCH>();
  // element k of row g leaves the tile: the closing product (inter-pass twiddle, or the post scale) and the store
  auto emit = [&](uint32_t k, const FrU& v_in) __attribute__((always_inline)) {
    FrU v = v_in;                                       // < 30p, limbs < 4*2^29
    const uint64_t go = out_base + k * P.out_xs + g * P.out_gs;
    TwU w;
    if (P.tw_full) {
      w = tab_load(twF + go);
    } else if (P.tw_mul != 0) {
      const uint64_t ex = P.tw_mul * k * (lo * G + g);
      v = ntt_post_mul(v, tab_load(twA + (ex >> P.tw_h)));
      w = tab_load(twB + (ex & ((1ull << P.tw_h) - 1)));
    } else if (P.post == 2) {
      v = ntt_post_mul2(v, tab_load(postA + (go >> P.post_h)), [&] { return tab_load(postB + (go & ((1ull << P.post_h) - 1))); });
      w = post_c;
    } else if (P.post == 3) {
      gstore(out + go, ntt_store_plain(v));
      return;
    } else if (P.post == 4) {
      w = tab_load(postA + k);
    } else if (P.post == 5) {                           // transforms without a full table: (minv * ginv^(row's first output index)) * (ginv^stride)^k
      v = ntt_post_mul(v, tab_load(postB + (go - (uint64_t)k * P.out_xs)));
      w = tab_load(postA + k);
    } else {
      w = post_c;
    }
    gstore(out + go, ntt_store_mul(v, w));
  };

  constexpr uint32_t S0 = LOG_NP & 1;
  FrU a, b, c, d;
  const bool direct = S0 == 0 && !P.load_x_fastest;    // (uniform)
  if (direct) {
    const uint32_t xr = bitrev(qf, LOG_NP - 2);         // element index = brev2(k) * np / 4 + brev(qf)
    a = fetch(in_base + (uint64_t)(xr) * P.in_xs + g * P.in_gs, xr);
    b = fetch(in_base + (uint64_t)(xr + 2u * (np >> 2)) * P.in_xs + g * P.in_gs, xr + 2u * (np >> 2));   // k = 1 -> brev2 = 2
    c = fetch(in_base + (uint64_t)(xr + 1u * (np >> 2)) * P.in_xs + g * P.in_gs, xr + 1u * (np >> 2));   // k = 2 -> brev2 = 1
    d = fetch(in_base + (uint64_t)(xr + 3u * (np >> 2)) * P.in_xs + g * P.in_gs, xr + 3u * (np >> 2));
  } else {
    for (uint32_t e = threadIdx.x; e < elems; e += blockDim.x) {
      uint32_t x, gg;
      if (P.load_x_fastest) { x = e & (np - 1); gg = e >> LOG_NP; }
      else { gg = e & (G - 1u); x = e >> log_g; }
      const uint64_t gi = in_base + x * P.in_xs + gg * P.in_gs;
      lds_store(lds, plane, gg * pitch + (swz_wl(bitrev(x, LOG_NP)) ^ row_term_wl(gg, G)), fetch(gi, x));
    }
    __syncthreads();
    if constexpr (S0 == 1) {                           // stage 0 alone (all twiddles one): two butterflies per lane, neighbours in the row
      const uint32_t x0 = qf << 2;
      a = lds_load(lds, plane, at(x0)); b = lds_load(lds, plane, at(x0 + 1)); c = lds_load(lds, plane, at(x0 + 2)); d = lds_load(lds, plane, at(x0 + 3));
      TwU w0{a, a};
      if (twisted) w0 = tab_load(stage_tab + 1);
      [[clang::always_inline]] bf(std::integral_constant<int, 0>{}, a, b, w0, !twisted);
      [[clang::always_inline]] bf(std::integral_constant<int, 0>{}, c, d, w0, !twisted);
      lds_store(lds, plane, at(x0), a); lds_store(lds, plane, at(x0 + 1), b); lds_store(lds, plane, at(x0 + 2), c); lds_store(lds, plane, at(x0 + 3), d);
      // pair 1 takes groups of 8 elements = two of these lanes' quadruples: inside the wave while it owns >= 8 elements per row
      if (8u <= own) wave_handover(); else __syncthreads();
    }
  }
  for_limbs<(int)(LOG_NP / 2)>([&](auto pc) {
    constexpr uint32_t s = S0 + 2u * (uint32_t) decltype(pc)::value;
    constexpr uint32_t m = 1u << s;
    constexpr bool first = decltype(pc)::value == 0, last = s + 2 == LOG_NP;
    const uint32_t j = qf & (m - 1), x0 = ((qf >> s) << (s + 2)) + j;
    const uint32_t ia = at(x0), ib = at(x0 + m), ic = at(x0 + 2 * m), id = at(x0 + 3 * m);
    if (!(first && direct)) { a = lds_load(lds, plane, ia); b = lds_load(lds, plane, ib); c = lds_load(lds, plane, ic); d = lds_load(lds, plane, id); }
    const bool one = !twisted && SCH::may_skip(s) && j == 0;
    {
      TwU w1{a, a};
      if (!one) w1 = tab_load(stage_tab + (twisted ? m + j : j << (LOG_NP - 1 - s)));   // (requesting it before the hand-over, to run under the wait: measured, nothing)
      [[clang::always_inline]] bf(std::integral_constant<int, (int)s>{}, a, b, w1, one);
      [[clang::always_inline]] bf(std::integral_constant<int, (int)s>{}, c, d, w1, one);
    }
    const bool one2 = !twisted && SCH::may_skip(s + 1) && j == 0;
    {
      TwU w2{a, a};
      if (!one2) w2 = tab_load(stage_tab + (twisted ? 2u * m + j : j << (LOG_NP - 2 - s)));
      [[clang::always_inline]] bf(std::integral_constant<int, (int)s + 1>{}, a, c, w2, one2);
    }
    {
      const TwU w3 = tab_load(stage_tab + (twisted ? 3u * m + j : (j + m) << (LOG_NP - 2 - s)));
      [[clang::always_inline]] bf(std::integral_constant<int, (int)s + 1>{}, b, d, w3, false);
    }
    if constexpr (!last) {
      lds_store(lds, plane, ia, a); lds_store(lds, plane, ib, b); lds_store(lds, plane, ic, c); lds_store(lds, plane, id, d);
      // the next pair's groups span 16 m elements of a row; the wave owns 256 / G of them
      if (16u * m <= own) wave_handover(); else __syncthreads();
    } else {
      emit(x0, a); emit(x0 + m, b); emit(x0 + 2 * m, c); emit(x0 + 3 * m, d);   // (last pair: x0 == j == qf)
    }
  });
}

// tab[j] = base^(j * step): the plain integer and its quotient (UTab)
__global__ void ntt_pow_table_kernel(UTab* tab, Fr base, uint64_t step, uint64_t count) {
  uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  tab_store(tab + j, tw_make(to_canonical(pow_u64(base, j * step))));
}

// tab[j] = c * base^j (c a Montgomery form)
__global__ void ntt_pow_scaled_table_kernel(UTab* tab, Fr base, Fr c, uint64_t count) {
  uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= count) return;
  tab_store(tab + j, tw_make(to_canonical(mul(pow_u64(base, j), c))));
}

// The inter-pass twiddles of a two-pass transform N = N_1 * S, laid out like the first pass's OUTPUT: full[k * S + col] = w^(k * col)
// (k < N_1, col < S), entries like every table's (UTab) -- from the two-level table w^e = A[e >> h] * B[e & mask].
__global__ void ntt_full_twiddle_kernel(UTab* __restrict__ full, const UTab* __restrict__ A, const UTab* __restrict__ B, uint32_t h,
                                        uint32_t log_s, uint64_t count) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint64_t k = i >> log_s, col = i & ((1ull << log_s) - 1), ex = k * col;
  const FrU w = ntt_tab_product(tab_load(A + (ex >> h)), tab_load(B + (ex & ((1ull << h) - 1))));   // < 2p, N
  tab_store(full + i, ntt_tab_entry(w));                                                    // canonical, and its quotient
}

// (round 5) The same table with the scale factors of a coset / inverse transform FOLDED in:
//   full[k * S + col] = w^(k * col) * pre^col * post_c * post^k
// The input twist pre^i of coset_fft (i = x * S + col: domain.rs:176-189) splits into pre^col -- constant over the first pass's
// sub-transform of column col, so it commutes with it and lands here -- and (pre^S)^x, ONE product by a table of N_1 entries at the
// load.  The output scale post_c * post^K of ifft / icoset_fft (K = k + N_1 * k2: domain.rs:163-173, 197-203) splits into
// post_c * post^k -- constant over the second pass's sub-transform of row k: here -- and (post^N_1)^k2, ONE product by a table of S
// entries at the last store.  coset_fft's first pass: two products less one; ifft's last pass: one less; icoset_fft's: three less one.
__global__ void ntt_full_folded_kernel(UTab* __restrict__ full, const UTab* __restrict__ A, const UTab* __restrict__ B, uint32_t h,
                                       uint32_t log_s, uint64_t count, const UTab* __restrict__ preA, const UTab* __restrict__ preB,
                                       uint32_t pre_h, const UTab* __restrict__ postA, const UTab* __restrict__ postB, uint32_t post_h,
                                       TwU post_c, int has_post_c) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= count) return;
  const uint64_t k = i >> log_s, col = i & ((1ull << log_s) - 1), ex = k * col;
  FrU w = ntt_tab_product(tab_load(A + (ex >> h)), tab_load(B + (ex & ((1ull << h) - 1))));   // < 2p, N (and so after every product below)
  if (preA != nullptr) w = ntt_tab_factor2(w, tab_load(preA + (col >> pre_h)), [&] { return tab_load(preB + (col & ((1ull << pre_h) - 1))); });
  if (postA != nullptr) w = ntt_tab_factor2(w, tab_load(postA + (k >> post_h)), [&] { return tab_load(postB + (k & ((1ull << post_h) - 1))); });
  if (has_post_c) w = ntt_tab_factor(w, post_c);
  tab_store(full + i, ntt_tab_entry(w));
}

// (round 5) The row twist (pre^S)^x of a coset transform's first pass folded into the butterflies: a DIT block of 2m = 2^(s+1) outputs at
// stage s is the transform of the row's samples at stride sigma = N_p / 2m, and  sum_t x_t h^(sigma t) w_2m^(t k)  =  E(k) + h^sigma w_2m^k O(k)
// with E, O the same sums over the even / odd samples (stride 2 sigma) -- so the twisted transform is the plain one with stage s's twiddle
// w_2m^j replaced by h^sigma w_2m^j, and no product at the load at all.  Stage-major table: tab[m + j] = h^sigma * w_p^(j sigma), j < m = 2^s
// (tab[0] unused).  The twiddle-one products of the early stages are no longer skipped (h^sigma != 1).
__global__ void ntt_stage_table_kernel(UTab* tab, Fr pre, uint64_t s_cols, Fr omega, uint64_t step0, uint32_t log_np) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (1u << log_np)) return;
  if (i == 0) { tab_store(tab, tw_make(to_canonical(Fr::one()))); return; }
  const uint32_t s = 31u - (uint32_t)__clz(i), m = 1u << s, j = i - m;
  const uint64_t sigma = (1ull << log_np) >> (s + 1);
  tab_store(tab + i, tw_make(to_canonical(mul(pow_u64(pre, s_cols * sigma), pow_u64(omega, step0 * j * sigma)))));
}

// a[i] *= c * gA[i >> h] * gB[i & mask]   (gA == nullptr: a[i] *= c);  c in the memory format
__global__ void ntt_scale_kernel(Fr* a, uint64_t n, Fr c, const UTab* __restrict__ gA, const UTab* __restrict__ gB, uint32_t h) {
  uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  FrU v = ntt_scale_const(ntt_load(gload(a + i)), c);                   // (c is a Montgomery form: c * 2^261, then the Montgomery product) < 2p
  if (gA != nullptr) v = ntt_scale_pow(v, tab_load(gA + (i >> h)), [&] { return tab_load(gB + (i & ((1ull << h) - 1))); });
  gstore(a + i, ntt_reduce_lt2p(v));
}

}  // namespace

}  // namespace zk

#include "ntt_tables.hpp"  // the table cache and the scratch pool: Key, PowTables, tables_make_room, build_pow_tables, build_folded, scratch_for, to_tw

namespace zk {

namespace {

// ONE table of the pass kernels, by (kind, LOG_NP): rows of 2^1 .. 2^12 for the two barrier kernels, 2^8 .. 2^12 for the wave-local one.
// One instantiation per row length: static stage loops.  ntt_configure walks it, the launcher indexes it.
using NttPassKernel = void (*)(const Fr*, Fr*, NttPassParams, const UTab*, const UTab*, const UTab*, const UTab*, const UTab*, const UTab*, const UTab*, TwU,
                               const UTab*, NttBatch);
constexpr NttPassKernel g_ntt_kernels[NTT_KERNEL_KINDS][NTT_MAX_LOG_NP + 1] = {
    // [kind][LOG_NP]; no kernel for LOG_NP == 0, nor for wave-local rows shorter than 2^8
    {nullptr, ntt_pass_kernel<1, false>, ntt_pass_kernel<2, false>, ntt_pass_kernel<3, false>, ntt_pass_kernel<4, false>, ntt_pass_kernel<5, false>,
     ntt_pass_kernel<6, false>, ntt_pass_kernel<7, false>, ntt_pass_kernel<8, false>, ntt_pass_kernel<9, false>, ntt_pass_kernel<10, false>,
     ntt_pass_kernel<11, false>, ntt_pass_kernel<12, false>},
    {nullptr, ntt_pass_kernel<1, true>, ntt_pass_kernel<2, true>, ntt_pass_kernel<3, true>, ntt_pass_kernel<4, true>, ntt_pass_kernel<5, true>,
     ntt_pass_kernel<6, true>, ntt_pass_kernel<7, true>, ntt_pass_kernel<8, true>, ntt_pass_kernel<9, true>, ntt_pass_kernel<10, true>,
     ntt_pass_kernel<11, true>, ntt_pass_kernel<12, true>},
    {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, ntt_pass_wl_kernel<8>, ntt_pass_wl_kernel<9>, ntt_pass_wl_kernel<10>,
     ntt_pass_wl_kernel<11>, ntt_pass_wl_kernel<12>},
};

std::mutex g_cfg_mu;
std::map<int, int> g_cfg;  // device -> rc of its one-time kernel configuration

// the device pointer a planned table argument names
const UTab* ntt_table(NttTab t, const PowTables* T, const PowTables* Tpre, const PowTables* Tpost, const PowTables::Folded& F) {
  switch (t) {
    case NTT_TAB_T_A: return T->A;
    case NTT_TAB_T_B: return T->B;
    case NTT_TAB_T_FULL: return T->full;
    case NTT_TAB_TPRE_A: return Tpre->A;
    case NTT_TAB_TPRE_B: return Tpre->B;
    case NTT_TAB_TPOST_A: return Tpost->A;
    case NTT_TAB_TPOST_B: return Tpost->B;
    case NTT_TAB_F_FULL: return F.full;
    case NTT_TAB_F_PRE_ROWS: return F.pre_rows;
    case NTT_TAB_F_PRE_STAGES: return F.pre_stages;
    case NTT_TAB_F_PRE_COLS: return F.pre_cols;
    case NTT_TAB_F_POST_ROWS: return F.post_rows;
    case NTT_TAB_F_POST_ROWC: return F.post_rowc;
    case NTT_TAB_F_TW_B_SCALED: return F.tw_b_scaled;
    default: return nullptr;
  }
}

}  // namespace

// the tile kernels stage up to 4096 x 36 B = 144 KiB in dynamic LDS (gfx950: 160 KiB per CU)
int ntt_configure() {
  int dev = 0;
  ZK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_cfg_mu);  // the attribute is per device: once for every device this process drives
  auto it = g_cfg.find(dev);
  if (it != g_cfg.end()) return it->second;
  int rc = ZK_OK;
  for (const auto& kind : g_ntt_kernels)
    for (NttPassKernel fn : kind) {
      if (fn == nullptr) continue;
      hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize, (int)NTT_LDS_BYTES_MAX);
      if (e != hipSuccess) {
        std::fprintf(stderr, "[mi355zk] hipFuncSetAttribute(ntt pass kernel, 160 KiB LDS) failed: %s\n", hipGetErrorString(e));
        rc = ZK_ERR_DEVICE;
      }
    }
  g_cfg[dev] = rc;
  return rc;
}

int ntt_scale(Fr* d_a, uint32_t log_n, const Fr& c, const Fr* g, hipStream_t st);

// d_a: 2^log_n Fr elements on the current device, in place:
//   a[i] *= pre_g^i (if pre_g)  ->  X[k] = sum_i a[i] * omega^(i*k)  ->  X[k] *= post_c * post_g^k (if given).
int ntt_run_batch(Fr* const* d_arrays, uint32_t batch, uint32_t log_n, const Fr& omega, const Fr* pre_g, const Fr* post_c, const Fr* post_g, hipStream_t st);
int ntt_run_scaled(Fr* d_a, uint32_t log_n, const Fr& omega, const Fr* pre_g, const Fr* post_c, const Fr* post_g, hipStream_t st) {
  return ntt_run_batch(&d_a, 1, log_n, omega, pre_g, post_c, post_g, st);
}

// (round 5) `batch` (1 .. NTT_MAX_BATCH) independent transforms of the same size and kind (prover.rs:217-241 runs ifft and coset_fft on a, b and
// c), every pass ONE launch over all their tiles.  Why: a 2^20 pass is 512 workgroups on 512 workgroup slots -- every CU loads, then computes,
// then stores, and the load and store phases (~15 of a pass's 47 - 55 us) hide behind nothing.  With the tiles of the next transform queued in
// the same launch a CU starts loading them while its other workgroup still computes: 2^20 fft 0.105 -> 0.087 ms per transform for batch = 2 .. 3
// (tools/exp_ntt_streams.py measured the same with one stream per transform: profiles/r05_ntt_batch.txt).
// What runs is decided by ntt_plan (ntt_plan.hpp); here the plan's tables are found or built, its scratch leased and its passes launched.
int ntt_run_batch(Fr* const* d_arrays, uint32_t batch, uint32_t log_n, const Fr& omega, const Fr* pre_g, const Fr* post_c, const Fr* post_g, hipStream_t st) {
  if (batch == 0 || batch > NTT_MAX_BATCH || d_arrays == nullptr) return ZK_ERR_BAD_ARGS;
  for (uint32_t t = 0; t < batch; ++t)
    if (d_arrays[t] == nullptr) return ZK_ERR_BAD_ARGS;
  if (log_n == 0) {
    // single element: X[0] = a[0] * post_c
    if (post_c == nullptr) return 0;
    for (uint32_t t = 0; t < batch; ++t) {
      int rc0 = ntt_scale(d_arrays[t], 0, *post_c, nullptr, st);
      if (rc0) return rc0;
    }
    return 0;
  }
  NttRequest Q;
  Q.log_n = log_n;
  Q.batch = batch;
  Q.pre_g = pre_g != nullptr;
  Q.post_c = post_c != nullptr;
  Q.post_g = post_g != nullptr;
  NttPlan N;
  // planned first: pure arithmetic, so a refused request (log_n > 30) returns, as it always did, before anything touches the device or the
  // caches.  (The first call therefore reads every NTT knob, MI355ZK_NTT_TABLES_GB included, here, before the device is touched.)
  int rc = ntt_plan(Q, ntt_knobs(), &N);
  if (rc) return rc;
  rc = ntt_configure();
  if (rc) return rc;
  // held from the table lookup to the last launch: the table cache may be dropped (when full) only while nobody is between
  // "got a table pointer" and "enqueued the kernels that read it"
  std::lock_guard<std::mutex> run_lk(g_run_mu);
  rc = tables_make_room(3);
  if (rc) return rc;
  PowTables* T = nullptr;
  PowTables* Tpre = nullptr;
  PowTables* Tpost = nullptr;
  rc = build_pow_tables(st, log_n, omega, true, N.b, N.R, &T, N.full_log_s);
  if (rc) return rc;
  if (N.want_tpre) { rc = build_pow_tables(st, log_n, *pre_g, false, nullptr, 0, &Tpre); if (rc) return rc; }
  if (N.want_tpost) { rc = build_pow_tables(st, log_n, *post_g, false, nullptr, 0, &Tpost); if (rc) return rc; }
  const TwU post_cu = post_c ? to_tw(*post_c) : (post_g ? to_tw(Fr::one()) : TwU{FrU::zero(), FrU::zero()});   // (neither: post == 3 multiplies by nothing)
  PowTables::Folded F;
  if (N.want_folded) { rc = build_folded(st, log_n, omega, T, Tpre, Tpost, pre_g, post_c, post_cu, post_g, N.b, N.R, N.fold, &F); if (rc) return rc; }
  static const int slot_pass = prof_slot("ntt_pass");
  Fr* scratch = nullptr;
  if (N.want_scratch) {
    int dev = 0;
    ZK_HIP(hipGetDevice(&dev));
    rc = scratch_for(dev, st, (sizeof(Fr) << log_n) * batch, &scratch);
    if (rc) return rc;
  }

  for (int p = 0; p < N.R; ++p) {
    const NttPass& pass = N.pass[p];
    NttBatch BP{};
    for (uint32_t t = 0; t < batch; ++t) {
      BP.in[t] = pass.src == NTT_BUF_ARRAY ? d_arrays[t] : scratch + ((uint64_t)t << log_n);
      BP.out[t] = pass.dst == NTT_BUF_ARRAY ? d_arrays[t] : scratch + ((uint64_t)t << log_n);
    }
    const UTab* tab[NTT_ARGS];
    for (uint32_t a = 0; a < NTT_ARGS; ++a) tab[a] = ntt_table(pass.tab[a], T, Tpre, Tpost, F);
    prof_begin(slot_pass, st);
    hipLaunchKernelGGL(g_ntt_kernels[pass.kind][pass.P.log_np], dim3(pass.grid), dim3(pass.threads), pass.lds_bytes, st, BP.in[0], BP.out[0], pass.P,
                       T->roots[pass.P.log_np], tab[NTT_ARG_TW_A], tab[NTT_ARG_TW_B], tab[NTT_ARG_PRE_A], tab[NTT_ARG_PRE_B], tab[NTT_ARG_POST_A],
                       tab[NTT_ARG_POST_B], post_cu, tab[NTT_ARG_TW_F], BP);
    ZK_HIP(hipGetLastError());
    prof_end(slot_pass, st);
  }
  return 0;
}

int ntt_run(Fr* d_a, uint32_t log_n, const Fr& omega, hipStream_t st) { return ntt_run_scaled(d_a, log_n, omega, nullptr, nullptr, nullptr, st); }

// a[i] *= c * g^i  (g == nullptr: a[i] *= c): standalone elementwise form of distribute_powers
// (domain.rs:176-189) / the ifft scaling (domain.rs:163-173); the domain ops use the fused forms above.
int ntt_scale(Fr* d_a, uint32_t log_n, const Fr& c, const Fr* g, hipStream_t st) {
  const uint64_t n = 1ull << log_n;
  const UTab* A = nullptr;
  const UTab* B = nullptr;
  uint32_t h = 0;
  std::lock_guard<std::mutex> run_lk(g_run_mu);
  if (g != nullptr && log_n > 0) {
    PowTables* T = nullptr;
    int rc = tables_make_room(1);
    if (rc) return rc;
    rc = build_pow_tables(st, log_n, *g, false, nullptr, 0, &T);
    if (rc) return rc;
    A = T->A;
    B = T->B;
    h = T->h;
  }
  static const int slot_scale = prof_slot("ntt_scale");
  prof_begin(slot_scale, st);
  hipLaunchKernelGGL(ntt_scale_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d_a, n, c, A, B, h);
  ZK_HIP(hipGetLastError());
  prof_end(slot_scale, st);
  return 0;
}

}  // namespace zk
