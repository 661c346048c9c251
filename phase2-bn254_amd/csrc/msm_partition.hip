// The group-independent stages of the Pippenger pipeline (msm_impl.hpp has the design): the digit kernels (stage 1), the partition
// (stage 2), the size order of the buckets (stage 3) and the plan of the heavy path, with the host functions that launch them
// (msm_partition.hpp).  No kernel here touches a curve point, so there is ONE copy of them for G1 and G2: msm_g1.hip and msm_g2.hip
// call the launchers below.  (No ZK_CHAIN_MAD: the only field operation here is the digit kernels' to_canonical.)
#include "msm_partition.hpp"

#include <map>
#include <mutex>
#include <vector>

#include "field.hpp"
#include "msm_digits.hpp"

namespace zk {

std::atomic<int> g_msm_inflight[16];

namespace {

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

// The plain digit kernel over a BATCH of exponent vectors that share the base vector and the density map (MsmRequest::n_vectors): the
// vector on blockIdx.y, exponent i of vector v at scalars + (v * scalar_stride + i) * 8, its G.W keys on the planes v * G.W + w -- the
// partition and everything behind it then see n_vectors * G.W windows of ONE call.  Same block as the plain kernel: a wave reads 64
// consecutive 32-byte exponents (2 KiB, two 16-byte loads per lane) and writes 256 consecutive bytes per key plane; the grid is
// (ceil(kstride / 256), n_vectors), so a short vector still brings n_vectors times the workgroups of its single call.  The density word
// of exponent i is one load per lane, the same word for every v.  The non-canonical-exponent word takes the lowest INDEX over all
// vectors: the call only needs to know that some vector has one (msm_device_batch then runs that pass's vectors one by one).
template <uint32_t RM>
__global__ void __launch_bounds__(256) msm_digits_batch_kernel(const uint32_t* __restrict__ scalars, uint64_t n, uint64_t scalar_stride,
                                                              const uint32_t* __restrict__ density, MsmGeom G, int scalars_mont, uint64_t kstride,
                                                              uint32_t* __restrict__ keys, unsigned long long* __restrict__ err_scalar) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t WD = G.W;
  uint32_t* __restrict__ kv = keys + (uint64_t)blockIdx.y * WD * kstride;   // plane 0 of this vector
  if (i >= n) {
    // the (at most three) slots between the key planes: "no bucket", as the plain kernel leaves them
    if (i < kstride) for (uint32_t w = 0; w < WD; ++w) kv[(uint64_t)w * kstride + i] = G.nb;
    return;
  }
  bool active = true;
  if (density != nullptr) active = (density[i >> 5] >> (i & 31)) & 1;
  uint32_t s[9];
  const uint4* sp = reinterpret_cast<const uint4*>(scalars + ((uint64_t)blockIdx.y * scalar_stride + i) * 8);
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
    atomicMin(err_scalar, (unsigned long long)i);
    active = false;
  }
  if (!active || any == 0) {
    for (uint32_t w = 0; w < WD; ++w) kv[(uint64_t)w * kstride + i] = G.nb;
    return;
  }
  msm_scalar_digits<RM>(s, G, 0u, WD, [&](uint32_t w, uint32_t d, uint32_t neg) {
    if (w < WD) kv[(uint64_t)w * kstride + i] = d ? ((d - 1) | neg) : G.nb;
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


// 3. buckets ordered by size (descending) so that the 64 lanes of a wave own buckets of (nearly) equal length --
//    bucket sizes are Poisson distributed and a wave runs as long as its longest lane -- and so that the few very
//    long buckets of a skewed input come first.  A counting sort on the size (exact below 2048, then in steps of
//    2048): histogram, suffix scan, scatter; the order inside a bin is irrelevant.
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

// The plan of the heavy path (stage 4a, msm_impl.hpp: msm_accumulate_heavy_kernel / msm_heavy_combine_kernel read it).
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

// the index list of the identity order (segsum_device)
__global__ void __launch_bounds__(256) msm_iota_kernel(uint32_t* __restrict__ v, uint32_t n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) v[i] = i;
}

std::mutex g_part_cfg_mu;
std::map<int, int> g_part_cfg;  // device -> the return code of its configuration

}  // namespace

int part_configure(int dev) {
  std::lock_guard<std::mutex> lk(g_part_cfg_mu);
  auto it = g_part_cfg.find(dev);
  if (it != g_part_cfg.end()) return it->second;
  int rc = ZK_OK;
  std::vector<const void*> fns = {reinterpret_cast<const void*>(msm_scatter_kernel), reinterpret_cast<const void*>(msm_bucket_kernel),
                                  reinterpret_cast<const void*>(msm_bigbin_place_kernel)};
  for (uint32_t rmul : {1u, 3u, 5u, 7u, 9u, 11u, 13u, 15u}) ZK_DISPATCH_RMUL(rmul, fns.push_back(reinterpret_cast<const void*>(msm_digits_hist_kernel<RM>)));
  for (const void* fn : fns) {
    hipError_t e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    if (e != hipSuccess) {
      std::fprintf(stderr, "[mi355zk] hipFuncSetAttribute(partition kernel, 160 KiB LDS) failed: %s\n", hipGetErrorString(e));
      rc = ZK_ERR_DEVICE;
    }
  }
  g_part_cfg[dev] = rc;
  return rc;
}

int msm_checkpoint(const MsmPartCall& A, const char* what, const ChunkPlan& C) {
  if (!A.knobs.debug) return 0;
  const MsmPlan& P = A.plan;
  ZK_HIP(hipStreamSynchronize(A.st));
  std::fprintf(stderr, "[mi355zk] msm<%d> n=%llu chunk@%llu+%llu c=%u W=%u buckets=%u levels=%u part(lo=%u nbin=%u st=%u): %s done\n", A.group,
               (unsigned long long)A.n, (unsigned long long)C.lo, (unsigned long long)C.n, P.G.c, P.WL, P.n_buckets, P.n_levels, C.P.lo_bits, C.P.nbin,
               C.P.st, what);
  return 0;
}

void msm_order_by_size(const uint32_t* first, const uint32_t* last, uint32_t n_buckets, uint32_t* hist, uint32_t* order, uint32_t* sizes_sorted,
                       hipStream_t st) {
  uint32_t hb = (n_buckets + 4095) / 4096;
  hipLaunchKernelGGL(msm_size_hist_kernel, dim3(hb < 1024 ? hb : 1024), dim3(1024), 0, st, first, last, n_buckets, hist);
  hipLaunchKernelGGL(msm_size_scan_kernel, dim3(1), dim3(1024), 0, st, hist);
  hipLaunchKernelGGL(msm_size_scatter_kernel, dim3((n_buckets + 1024 * MSM_SCATTER_PER - 1) / (1024 * MSM_SCATTER_PER)), dim3(1024), 0, st, first,
                     last, n_buckets, hist, order, sizes_sorted);
}

void launch_heavy_plan(hipStream_t st, const uint32_t* sizes_sorted, uint32_t hb, uint32_t heavy, uint32_t seg, uint32_t* item_off) {
  hipLaunchKernelGGL(msm_heavy_plan_kernel, dim3(1), dim3(1024), 0, st, sizes_sorted, hb, heavy, seg, item_off);
}

void launch_iota(hipStream_t st, uint32_t* v, uint32_t n) {
  hipLaunchKernelGGL(msm_iota_kernel, dim3((n + 255) / 256), dim3(256), 0, st, v, n);
}

int launch_digits(const MsmPartCall& A, const MsmPartWs& W, const ChunkPlan& C, const uint32_t* d_sc) {
  const MsmPlan& P = A.plan;
  const MsmGeom& G = P.G;
  const PartGeom& PG = C.P;
  const hipStream_t st = A.st;
  const uint64_t nc = C.n, kstride = (nc + 3) & ~3ull;  // distance between the key planes of two windows
  const uint32_t ncell = C.ncell, WL = P.WL;
  // density words and prefix ranks of this chunk's exponents (cuts are multiples of 32); under FullDensity exponent i of the
  // chunk owns base base_offset + lo + i
  const uint32_t* dens = A.d_density ? A.d_density + (C.lo >> 5) : nullptr;
  if (!C.small_scan) ZK_HIP(hipMemsetAsync(W.size_hist, 0, MSM_SIZE_BINS * 4, st));   // (msm_scan_small_kernel clears it)
  if (C.np > BIG_SEG) ZK_HIP(hipMemsetAsync(W.gcnt, 0, P.L.big_col - P.L.gcnt, st));  // gcnt and gcur (big bins only: see the bucket pass)
  prof_begin(msm_slots().digits, st);
  if (P.n_vectors > 1) {
    // a batch (msm_device_batch): d_sc is vector 0; the tile histograms, like everything behind them, run over WL = n_vectors * WD planes
    if (A.knobs.fused_a || P.tmode || A.scalar_stride < nc || P.n_vectors > 65535u) return (int)ZK_ERR_BAD_ARGS;
    ZK_DISPATCH_RMUL(G.rmul, hipLaunchKernelGGL(msm_digits_batch_kernel<RM>, dim3((unsigned)((kstride + 255) / 256), P.n_vectors), dim3(256), 0, st, d_sc, nc,
                                                A.scalar_stride, dens, G, A.scalars_mont ? 1 : 0, kstride, W.keys, W.d_err + 1));
    hipLaunchKernelGGL(msm_tile_hist_kernel, dim3(PG.n_st * WL), dim3(PART_THREADS), (size_t)PG.nbin * 4, st, W.keys, C.np, kstride, G.nb, WL, PG, W.tile_hist);
  } else if (!A.knobs.fused_a) {
    ZK_DISPATCH_RMUL(G.rmul, hipLaunchKernelGGL(msm_digits_plain_kernel<RM>, dim3((unsigned)((kstride + 255) / 256)), dim3(256), 0, st, d_sc, nc, dens, G,
                                                P.w_lo, P.w_hi, A.scalars_mont ? 1 : 0, kstride, W.keys, W.d_err + 1, C.lo));
    hipLaunchKernelGGL(msm_tile_hist_kernel, dim3(PG.n_st * WL), dim3(PART_THREADS), (size_t)PG.nbin * 4, st, W.keys, C.np, P.tmode ? C.np : kstride, G.nb, WL, PG,
                       W.tile_hist);
  } else {
    if (P.tmode) return (int)ZK_ERR_BAD_ARGS;
    int cus = 256;
    (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, A.dev);
    const uint32_t per_cu = (size_t)((ncell + 1) / 2) * 4 <= PART_LDS_A ? 2u : 1u;     // 1024-lane workgroups per CU (LDS histograms)
    const uint32_t grid = PG.n_st < per_cu * (uint32_t)cus ? PG.n_st : per_cu * (uint32_t)cus;
    ZK_DISPATCH_RMUL(G.rmul, hipLaunchKernelGGL(msm_digits_hist_kernel<RM>, dim3(grid), dim3(PART_THREADS), (size_t)((ncell + 1) / 2) * 4, st, d_sc, nc,
                                                dens, G, P.w_lo, P.w_hi, A.scalars_mont ? 1 : 0, PG, kstride, W.keys, W.tile_hist, W.d_err + 1, C.lo));
  }
  ZK_HIP(hipGetLastError());
  prof_end(msm_slots().digits, st);
  if (msm_checkpoint(A, "digits", C)) return ZK_ERR_DEVICE;
  return ZK_OK;
}

// ("msm_sort" spans the whole partition after the digits (scan + scatter + bucket + size order), as it did for the library sort)
int launch_partition(const MsmPartCall& A, const MsmPartWs& W, const ChunkPlan& C) {
  const MsmPlan& P = A.plan;
  const MsmGeom& G = P.G;
  const PartGeom& PG = C.P;
  const MsmSlots& S = msm_slots();
  const hipStream_t st = A.st;
  const uint64_t nc = C.n, kstride = (nc + 3) & ~3ull;
  const uint32_t ncell = C.ncell, WL = P.WL;
  const uint32_t* dens = A.d_density ? A.d_density + (C.lo >> 5) : nullptr;
  const uint32_t* dpre = A.d_dprefix ? A.d_dprefix + (C.lo >> 5) : nullptr;
  const uint64_t boff = A.base_offset + (A.d_density ? 0 : C.lo);
  prof_begin(S.sort, st);
  prof_begin(S.scan, st);
  if (C.small_scan) {
    hipLaunchKernelGGL(msm_scan_small_kernel, dim3(1), dim3(PART_THREADS), 0, st, W.tile_hist, PG, ncell, G.nb, W.col_total, W.bin_start, W.out_start, W.tile_off,
                       W.size_hist, W.big_col, W.big_seg, W.big_plan);
  } else {
    hipLaunchKernelGGL(msm_colsum_kernel, dim3((ncell + 255) / 256, PG.n_chunk), dim3(256), 0, st, W.tile_hist, PG, ncell, W.csum);
    hipLaunchKernelGGL(msm_colscan_kernel, dim3((ncell + 255) / 256), dim3(256), 0, st, W.csum, PG, ncell, W.col_total);
    hipLaunchKernelGGL(msm_binscan_kernel, dim3(1), dim3(PART_THREADS), 0, st, W.col_total, PG, ncell, G.nb, W.bin_start, W.out_start);
    hipLaunchKernelGGL(msm_tileoff_kernel, dim3((ncell + 255) / 256, PG.n_chunk), dim3(256), 0, st, W.tile_hist, W.csum, W.bin_start, PG, ncell, W.tile_off);
  }
  ZK_HIP(hipGetLastError());
  prof_end(S.scan, st);
  prof_begin(S.scatter, st);
  hipLaunchKernelGGL(msm_scatter_kernel, dim3(PG.n_st * WL), dim3(PART_THREADS), (size_t)(2 * ((PG.nbin + 3u) & ~3u) + 32) * 4 + (size_t)PG.st * 8, st,
                     W.keys, C.np, P.tmode ? C.np : kstride, boff, dens, dpre, G.nb, WL, PG, A.knobs.part_xcds, W.tile_off, W.pairs, P.tmode ? kstride : 0ull,
                     A.table_stride);
  ZK_HIP(hipGetLastError());
  prof_end(S.scatter, st);
  if (msm_checkpoint(A, "scatter", C)) return ZK_ERR_DEVICE;
  prof_begin(S.bucket, st);
  {
    const uint32_t nfl = (1u << PG.lo_bits) < 4 ? 4 : (1u << PG.lo_bits);
    const size_t fixed = (size_t)(2 * nfl + 32) * 4;
    // staging for the expected bin population with slack, at most what the CU has
    uint64_t want = (uint64_t)(C.np / PG.nbin) * 5 / 4 + 3ull * nfl + 4096;
    const uint64_t cap_max = (PART_LDS_MAX - fixed) / 4;
    if (want > cap_max) want = cap_max;
    if (want > (uint64_t)PART_EC * PART_THREADS + 3ull * nfl) want = (uint64_t)PART_EC * PART_THREADS + 3ull * nfl;
    const uint32_t stage_cap = (uint32_t)want & ~3u;
    hipLaunchKernelGGL(msm_bucket_kernel, dim3(ncell), dim3(PART_THREADS), fixed + (size_t)stage_cap * 4, st, W.pairs, W.bin_start, W.out_start, G.nb, PG,
                       stage_cap, W.first, W.last, W.vals_b);
    // the big bins (none for uniform exponents up to 2^26 points: the surplus workgroups of these launches exit at once).  A
    // chunk with at most BIG_SEG elements per window cannot have one at all -- the bucket kernel took every bin -- so a short call
    // does not pay for three idle launches (~5 us each of a 0.4-ms call at 2^10 .. 2^15 points)
    if (C.np > BIG_SEG) {
      const uint32_t max_seg = (uint32_t)(2 * (C.m / BIG_SEG) + 2);
      if (!C.small_scan) hipLaunchKernelGGL(msm_bigbin_plan_kernel, dim3(1), dim3(PART_THREADS), 0, st, W.bin_start, ncell, W.big_col, W.big_seg, W.big_plan);
      // (small grids: when there is no big bin -- uniform exponents -- the launches only cost their workgroups' start-up, and the
      // place kernel's LDS allows one workgroup per CU anyway)
      int n_cu = 256;
      (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, A.dev);
      const uint32_t big_grid = max_seg < 2u * (uint32_t)n_cu ? max_seg : 2u * (uint32_t)n_cu;
      const uint32_t place_grid = max_seg < (uint32_t)n_cu ? max_seg : (uint32_t)n_cu;
      hipLaunchKernelGGL(msm_bigbin_count_kernel, dim3(big_grid), dim3(PART_THREADS), (size_t)nfl * 4, st, W.pairs, W.bin_start, W.big_plan, W.big_col, W.big_seg,
                         G.nb, PG, W.gcnt);
      const size_t place_fixed = (size_t)(4 * nfl + 32) * 4, place_staged = place_fixed + (size_t)BIG_SEG * 4;
      const int staged = place_staged <= PART_LDS_MAX ? 1 : 0;
      hipLaunchKernelGGL(msm_bigbin_place_kernel, dim3(staged ? place_grid : big_grid), dim3(PART_THREADS), staged ? place_staged : place_fixed, st, W.pairs,
                         W.bin_start, W.out_start, W.big_plan, W.big_col, W.big_seg, G.nb, PG, staged, W.gcnt, W.gcur, W.first, W.last, W.vals_b);
    }
  }
  ZK_HIP(hipGetLastError());
  prof_end(S.bucket, st);
  if (msm_checkpoint(A, "bucket", C)) return ZK_ERR_DEVICE;
  msm_order_by_size(W.first, W.last, P.n_buckets, W.size_hist, W.order, W.sizes_b, st);
  ZK_HIP(hipGetLastError());
  prof_end(S.sort, st);
  if (msm_checkpoint(A, "partition", C)) return ZK_ERR_DEVICE;
  return ZK_OK;
}

void msm_geometry(uint64_t n, uint32_t wgroups, uint32_t* c, uint32_t* W) {
  MsmGeom G = choose_geom(n, 1, wgroups ? wgroups : 1, msm_knobs());
  *c = G.c;
  *W = G.W;
}

// a batch of n_vectors vectors of n exponents (msm_device_batch): the windows of one vector and the vectors one pipeline pass takes
void msm_batch_geometry(uint64_t n, uint32_t n_vectors, int group, uint32_t* max_windows, uint32_t* W, uint32_t* vectors_per_pass) {
  *max_windows = MSM_BATCH_MAX_WINDOWS;
  const MsmKnobs K = msm_knobs();
  const MsmGeom G = choose_geom(n, group, 1, K);
  *W = G.W;
  *vectors_per_pass = msm_batch_split(n, n_vectors, G, group, K);
}

// table mode (msm_device): the window layout a table of n_bases points is built for -- width[w] bits per window, window w scaled by
// 2^(width[0] + .. + width[w-1])
void msm_table_geometry(uint64_t n_bases, int group, uint32_t* c, uint32_t* W, uint8_t width[64]) {
  const MsmGeom G = make_geom(table_window_bits(n_bases, group, msm_knobs()));
  *c = G.c;
  *W = G.W;
  if (width) for (uint32_t w = 0; w < 64; ++w) width[w] = w < G.W ? G.width[w] : 0;
}

// host self-test hook for the digit extraction (tests/test_msm_digits_host.py): the signed digits of one scalar for the geometry
// chosen for (n, wgroups), windows [w_start, w_stop) -- direct != 0: the way a window-group rank computes them (chain started one
// window below w_start, fallback on the sign boundary), direct == 0: the plain chain from window 0.  digits[w] = signed digit
// (0 = no bucket) for the windows produced, INT32_MIN elsewhere; geom = {c, W, nb, rmul, rshift, width[0..W), shift[0..W)}.
int msm_selftest_digits(uint64_t n, uint32_t wgroups, const uint32_t scalar[8], uint32_t w_start, uint32_t w_stop, int direct, int32_t* digits,
                        uint32_t* geom) {
  const MsmGeom G = choose_geom(n, 1, wgroups ? wgroups : 1, msm_knobs());
  if (G.W == 0) return ZK_ERR_BAD_ARGS;
  if (geom) {
    geom[0] = G.c; geom[1] = G.W; geom[2] = G.nb; geom[3] = G.rmul; geom[4] = G.rshift;
    for (uint32_t w = 0; w < G.W; ++w) { geom[5 + w] = G.width[w]; geom[5 + G.W + w] = G.shift[w]; }
  }
  if (!digits || !scalar) return ZK_OK;
  if (w_stop > G.W) w_stop = G.W;
  uint32_t s[9];
  for (int l = 0; l < 8; ++l) s[l] = scalar[l];
  s[8] = 0;
  for (uint32_t w = 0; w < G.W; ++w) digits[w] = INT32_MIN;
  auto emit = [&](uint32_t w, uint32_t d, uint32_t neg) { digits[w] = neg ? -(int32_t)d : (int32_t)d; };
  auto from0 = [&](uint32_t w, uint32_t d, uint32_t neg) { if (w >= w_start) emit(w, d, neg); };
  if (direct) { ZK_DISPATCH_RMUL(G.rmul, msm_scalar_digits<RM>(s, G, w_start, w_stop, emit)); }
  else { ZK_DISPATCH_RMUL(G.rmul, (void)msm_scalar_digits_from<RM>(s, G, 0, w_stop, from0)); }
  return ZK_OK;
}

}  // namespace zk
