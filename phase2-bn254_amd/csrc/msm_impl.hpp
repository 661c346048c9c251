#pragma once
// Pippenger multi-scalar multiplication over BN254 G1 / G2 for gfx950 (MI355X).
//
// Replaces, behind the C ABI of include/mi355zk.h, the reference's
//   bellman/src/multiexp.rs:330-355  multiexp()          (window choice, density contract)
//   bellman/src/multiexp.rs:53-157   multiexp_inner()    (bucket fill, summation by parts, window join)
//   bellman/src/source.rs:36-70      (Arc<Vec<G>>, usize) Source: cursor + error semantics
// and the group law underneath (pairing/src/bn256/ec.rs:301-536).
//
// MI355X design (DESIGN.md "MSM"), not the reference's one-thread-per-window scan; every stage names the file it lives in:
//   1. digits      msm_digits.hpp (the digit chain, __host__ __device__), msm_partition.hip (the kernels)
//      msm_digits_plain_kernel  every scalar -> W signed digits (power-of-two or mixed-radix windows), written window-major as
//      msm_tile_hist_kernel     4-byte keys; per (window, super-tile) a histogram of the keys over the coarse bins.
//   2. partition   msm_partition.hip (hand-written, no library sort): column scans of the tile histograms give every (super-tile,
//      window, bin) run its exact position; msm_scatter_kernel moves (key, base index) pairs into their bin through LDS;
//      msm_bucket_kernel sorts every bin by bucket in registers and writes the per-bucket index lists (bucket starts aligned to
//      4 entries) and bounds; msm_bigbin_* handle bins that skewed inputs overfill.  HBM-bound: 28 B per (point, window).
//   3. size order  msm_partition.hip
//      msm_size_*_kernel        counting sort of the buckets by size (wave-level load balance, heavy buckets first).
//   4. accumulate  this file (msm_heavy_plan_kernel, which has no curve type in it: msm_partition.hip)
//      msm_accumulate_kernel    ONE LANE PER BUCKET for all W * nb buckets at once, in size order: gathers its affine bases and
//                               folds them into a U-form XYZZ accumulator held in VGPRs (8M+2S per point) -- the dominant
//                               kernel; the identity-base check (source.rs:50-52) is fused in;
//      msm_accumulate_heavy / msm_heavy_combine   segment-parallel path for buckets that one lane would walk too long.
//   5. reduce      this file
//      msm_reduce_level_kernel  sum_k k*B_k per window by chunked running sums (levels), then
//      msm_tree_kernel          pairwise trees: plain sums of the levels' A[] and the bit decomposition of the rest;
//                               both on R-domain XYZZ records (curveu.hpp: U-form full additions).
//   6. join        msm_join.hpp (host)  ONE Horner pass over all partial sums, grouped by their power of two (multiexp.rs:146-154).
// The result is a group element; the reference compares/normalises projective points by value
// (ec.rs:45-85, 596-629), so parity is defined on the affine normalisation.
//
// This file is the part of the DEVICE side that is templated on the field of the curve: the kernels and device helpers of stages 4
// and 5 (and the two small kernels of the error path and of segsum_device), and nothing else; msm_g1.hip and msm_g2.hip each compile
// their instantiation of it.  Stages 1 - 3 never touch a curve point and are compiled once, in msm_partition.hip (interface:
// msm_partition.hpp).  The host side lives in msm_plan.hpp (geometry, schedules and the workspace layout of a call), msm_pools.hpp
// (workspaces and pinned buffers), msm_join.hpp (the window join) and msm_host.hpp (msm_device / segsum_device: the launch
// sequence); the structs and limits all of them use are in msm_common.hpp.
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

// (msm_heavy_plan_kernel, which scans ceil(size / SEG) over that prefix into item_off, has no curve type in it: msm_partition.hip)

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
// Segmented sum of affine points (msm_host.hpp: segsum_device): the normalisation of the row sums (the index list of the identity order is
// msm_partition.hip's msm_iota_kernel).
template <class F>
__global__ void __launch_bounds__(256) msm_to_affine_kernel(const XYZZ<F>* __restrict__ in, Affine<F>* __restrict__ out, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = xyzz_to_affine(load_vec(in + i));
}

}  // namespace

}  // namespace zk
