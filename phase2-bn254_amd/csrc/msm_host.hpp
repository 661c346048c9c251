#pragma once
// Host driver of the Pippenger pipeline: msm_device = plan (msm_plan.hpp) -> lease a workspace (msm_pools.hpp) -> per chunk
// digits / partition (msm_partition.hip, compiled once for both groups) / accumulate -> per base set reduce, copy back and join
// (msm_join.hpp); segsum_device, the segmented sum that reuses the accumulation.  The kernels launched from here are msm_impl.hpp's,
// the ones that depend on the group; msm_g1.hip / msm_g2.hip include this file once each.
#include <atomic>
#include <chrono>
#include <cstring>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "msm_impl.hpp"
#include "msm_join.hpp"
#include "msm_partition.hpp"
#include "msm_plan.hpp"
#include "msm_pools.hpp"

namespace zk {

namespace {

// What is left to configure per group: the tree kernel keeps 256 register-form sums in LDS (72 KiB for G2, above the 64 KiB a kernel
// gets without asking).  Once per device, after the shared partition kernels (msm_partition.hip: part_configure(dev)).
std::mutex g_part_cfg_mu;
std::map<int, int> g_part_cfg;
template <class F>
int part_configure(int dev) {
  std::lock_guard<std::mutex> lk(g_part_cfg_mu);
  auto it = g_part_cfg.find(dev);
  if (it != g_part_cfg.end()) return it->second;
  int rc = zk::part_configure(dev);  // (qualified: the shared, non-template one)
  hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(msm_tree_kernel<F>), hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
  if (e != hipSuccess) {
    std::fprintf(stderr, "[mi355zk] hipFuncSetAttribute(partition kernel, 160 KiB LDS) failed: %s\n", hipGetErrorString(e));
    rc = ZK_ERR_DEVICE;
  }
  g_part_cfg[dev] = rc;
  return rc;
}

// the call's workspace as typed pointers (MsmLayout's offsets over the leased buffer): the untyped part and the XYZZ records
template <class F>
struct MsmWs : MsmPartWs {
  XYZZ<F>*seg_sums, *buckets, *partA, *partS, *rc, *wsums, *sumtmp;
  static_assert(sizeof(XYZZ<F>) == (sizeof(F) == sizeof(Fq) ? 128 : 256), "msm_plan.hpp sizes the record regions by these");
  MsmWs(char* ws, const MsmLayout& L) : MsmPartWs(ws, L) {
    at(ws, seg_sums, L.seg_sums), at(ws, buckets, L.buckets), at(ws, partA, L.partA), at(ws, partS, L.partS), at(ws, rc, L.rc), at(ws, wsums, L.wsums);
    at(ws, sumtmp, L.sumtmp);
  }
};

// what every launch stage of one msm_device call sees: the group-independent context (msm_partition.hpp) and the group's own part
template <class F>
struct MsmCall : MsmPartCall {
  MsmWs<F> ws;
  bool dense;
};

// fn(A4, CARRY) with the two run-time switches of the accumulation kernels as std::bool_constants
template <class Fn>
void with_a4_carry(bool a4, bool carry, Fn&& fn) {
  auto with_carry = [&](auto A4) { if (carry) fn(A4, std::true_type{}); else fn(A4, std::false_type{}); };
  if (a4) with_carry(std::true_type{}); else with_carry(std::false_type{});
}

// ---- the segment-parallel path for the buckets longer than `heavy` among order[0 .. hb): plan, segment sums, sums per bucket
struct HeavyParams {
  uint32_t hb, heavy, seg, grid;
  int dense, carry;
};
template <class F>
int launch_heavy(hipStream_t st, const Affine<F>* bases, const uint32_t* vals, const uint32_t* first, const uint32_t* last, const uint32_t* order,
                 const uint32_t* sizes_b, uint32_t* item_off, XYZZ<F>* seg_sums, XYZZ<F>* buckets, unsigned long long* d_err, const HeavyParams& H) {
  launch_heavy_plan(st, sizes_b, H.hb, H.heavy, H.seg, item_off);
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(msm_accumulate_heavy_kernel<F>, dim3(H.grid), dim3(MSM_HEAVY_LANES), MSM_HEAVY_LANES * sizeof(typename BucketAcc<F>::type), st, bases, vals,
                     first, last, order, item_off, H.hb, H.seg, seg_sums, H.dense, d_err);
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(msm_heavy_combine_kernel<F>, dim3(H.hb < 2048 ? H.hb : 2048), dim3(64), 64 * sizeof(typename BucketAcc<F>::type), st, seg_sums, order, item_off,
                     H.hb, buckets, H.carry);
  ZK_HIP(hipGetLastError());
  return ZK_OK;
}

// ---- bucket accumulation of the partitioned chunk over one base vector; carry: the buckets continue an earlier chunk
template <class F>
int launch_accumulate(const MsmCall<F>& A, const ChunkPlan& C, const Affine<F>* bases_set, bool carry) {
  constexpr bool g2 = std::is_same<F, Fq2>::value;
  const MsmWs<F>& W = A.ws;
  const MsmKnobs& K = A.knobs;
  const hipStream_t st = A.st;
  const uint32_t n_buckets = A.plan.n_buckets;
  const int dense = A.dense ? 1 : 0;
  prof_begin(msm_slots().heavy, st);
  // (grid-stride over the segments that exist; a short call must not pay for thousands of empty workgroups)
  uint32_t heavy_grid = (uint32_t)((C.m >> 12) < 1024 ? 1024 : (C.m >> 12) > 16384 ? 16384 : (C.m >> 12));
  if (heavy_grid > C.max_items) heavy_grid = C.max_items;
  if (int rc = launch_heavy(st, bases_set, W.vals_b, W.first, W.last, W.order, W.sizes_b, W.item_off, W.seg_sums, W.buckets, W.d_err,
                            HeavyParams{C.hb, C.heavy, C.heavy_seg, heavy_grid, dense, carry ? 1 : 0}))
    return rc;
  prof_end(msm_slots().heavy, st);
  prof_begin(msm_slots().acc, st);
  const dim3 grid((n_buckets + 255) / 256), pgrid((uint32_t)((2ull * n_buckets + 255) / 256)), block(256);
  // the lane-per-bucket launch leaves out what another launch does: the heavy buckets (> C.heavy, among order[0 .. C.hb)), and for a
  // short call also the long ones (> C.split_t, among order[0 .. C.split_hb)), which a quad each walks
  const bool split = C.split_t != 0 && !carry;
  const uint32_t skip_len = split ? C.split_t : C.heavy, skip_hb = split ? std::max(C.split_hb, C.hb) : C.hb;
  if (split) {
    hipLaunchKernelGGL(msm_accumulate_split_kernel<F>, dim3((4 * C.split_hb + 255) / 256), dim3(256), 0, st, bases_set, W.vals_b, W.first, W.last, W.order,
                       C.split_t, C.heavy, C.hb, C.split_hb, W.buckets, dense, W.d_err);
    ZK_HIP(hipGetLastError());
  }
  // A PAIR of lanes per bucket (msm_accumulate_pair_kernel / _g1_kernel) while the bucket lanes do not fill the device several times
  // over: there a launch lasts as long as its lanes' chains of dependent additions, and the pair's chain is half as long.
  // G2 (<= 3 * 2^17 buckets, i.e. <= 2^18 points): 2^16 points accumulate 0.416 -> 0.312 ms, the call 1.27 -> 1.17; 2^12: 0.845 -> 0.82;
  // 2^18: 2.09 -> 2.04.  With >= 2^19 buckets both forms run at the multiplier's rate and the pair pays its ~280 moves / selects per
  // addition (2^20: 3.37 -> 3.48 ms, 2^22: 13.1 -> 13.7): tools/ab_g2_pair.sh, profiles/r04_ab_g2_pair.txt.
  // G1 (same gate: <= 2^17 points): the pair does 1782 multiplier instructions where the lane does 1467, but the chain is 891 deep:
  // accumulate 2^12 0.097 -> 0.079 ms, 2^15 0.085 -> 0.053, 2^16 0.139 -> 0.095, 2^17 0.192 -> 0.171; 2^18 (lanes) 0.272 vs 0.305,
  // 2^20 1.07 vs 1.27: tools/ab_g1_pair.sh, profiles/r04_ab_g1_pair.txt.
  // MsmKnobs::g2_pair / g1_pair = 0 / 1: never / always.
  const int pair_mode = g2 ? K.g2_pair : K.g1_pair;
  const bool pair = pair_mode < 0 ? n_buckets <= MSM_PAIR_MAX_BUCKETS : pair_mode != 0;
  // the one-lane G2 kernel at two waves per SIMD -- for a call that is ALONE on its device: beside the prover's other seven
  // multiexps the two-wave kernel fills every register of the SIMDs it runs on and their waves cannot share them (eight threads with
  // window tables at 2^20: 6.3 - 6.6 ms with one wave, 6.6 - 7.0 with two; alone: accumulate 3.36 -> 3.21 ms).
  // MsmKnobs::g2_waves = 1 / 2: always one / always two.
  const bool w2 = g2 && !pair && (K.g2_waves == 0 ? g_msm_inflight[A.dev & 15].load(std::memory_order_relaxed) <= 1 : K.g2_waves == 2);
  with_a4_carry(K.acc_a4, carry, [&](auto A4, auto CARRY) {  // (acc_a4 off: the 4-byte index walk, kept for the traffic comparison in profiles/)
    constexpr bool a4 = decltype(A4)::value, cy = decltype(CARRY)::value;
    auto go = [&](auto kern, dim3 g) {
      hipLaunchKernelGGL(kern, g, block, 0, st, bases_set, W.vals_b, W.first, W.last, W.order, skip_len, skip_hb, n_buckets, W.buckets, dense, W.d_err);
    };
    if constexpr (g2) {
      if (pair) go(msm_accumulate_pair_kernel<a4, cy>, pgrid);
      else if (w2) go(msm_accumulate_g2w2_kernel<a4, cy>, grid);
      else go(msm_accumulate_kernel<F, a4, cy>, grid);
    } else {
      if (pair) go(msm_accumulate_pair_g1_kernel<a4, cy>, pgrid);
      else go(msm_accumulate_kernel<F, a4, cy>, grid);
    }
  });
  ZK_HIP(hipGetLastError());
  prof_end(msm_slots().acc, st);
  if (msm_checkpoint(A, "accumulate", C)) return (int)ZK_ERR_DEVICE;
  return ZK_OK;
}

// ---- bucket reduction: the running-sum levels, then the tree launches that leave wsums[w * n_out + k]
//      (k < n_levels: sum of A of level k;  k >= n_levels: bit sum j = k - n_levels of the last array)
template <class F>
int launch_reduce(const MsmCall<F>& A) {
  const MsmPlan& P = A.plan;
  const MsmWs<F>& W = A.ws;
  const hipStream_t st = A.st;
  const uint32_t WL = P.WL, n_levels = P.n_levels, n_out = P.n_out, t_rows = P.t_rows, t_cols = P.t_cols;
  // quad additions in the parallelism-starved parts of the reduction (G1; MsmKnobs::quad_tail off for the comparison,
  // quad_max_chunks = the largest chunk count x windows a level may have to run four lanes per chunk)
  TreeJobs<F> J{};
  J.quad = A.knobs.quad_tail ? 1u : 0u;
  const XYZZ<F>* in = W.buckets;
  uint64_t o = 0;
  for (uint32_t lv = 0; lv < n_levels; ++lv) {
    uint32_t threads = P.lvl_chunks[lv] * WL;
    XYZZ<F>* LA = W.partA + o * WL;
    XYZZ<F>* LS = W.partS + o * WL;
    // a level with few chunks is a chain of 2L dependent additions per lane on a mostly idle device: four lanes per chunk
    // then (msm_reduce_level_quad_kernel, G1); a level that fills the device keeps the lane per chunk (less work in total)
    if (A.knobs.quad_tail && threads <= A.knobs.quad_max_chunks)
      hipLaunchKernelGGL(msm_reduce_level_quad_kernel<F>, dim3((4 * threads + 255) / 256), dim3(256), 0, st, in, P.lvl_cnt[lv], 1u << P.lvl_logl[lv],
                         lv == 0 ? 1u : 0u, WL, LA, LS);
    else
      hipLaunchKernelGGL(msm_reduce_level_kernel<F>, dim3((threads + 255) / 256), dim3(256), 0, st, in, P.lvl_cnt[lv], 1u << P.lvl_logl[lv],
                         lv == 0 ? 1u : 0u, WL, LA, LS);
    ZK_HIP(hipGetLastError());
    J.in[lv] = LA;
    J.cnt[lv] = J.stride[lv] = P.lvl_chunks[lv];
    J.bit[lv] = -1;
    in = LS;
    o += P.lvl_chunks[lv];
  }
  // jobs of the first tree launch: the levels' A[] (plain sums), then either the bit decomposition of the last array S (`in`)
  // or, with the 2-D tail, its row and column sums; the second launch then carries the bit decompositions of those
  auto plain = [&J](uint32_t j) { J.reps[j] = 1; J.rep_stride[j] = 0; J.elem_stride[j] = 1; J.limit[j] = 0xffffffffu; J.off[j] = 0; };
  for (uint32_t lv = 0; lv < n_levels; ++lv) plain(lv);
  uint32_t n_jobs = n_levels;
  if (!P.tail2d) {
    for (uint32_t j = 0; j < P.final_bits; ++j, ++n_jobs) {
      plain(n_jobs);
      J.in[n_jobs] = in;
      J.cnt[n_jobs] = J.stride[n_jobs] = P.final_cnt;
      J.bit[n_jobs] = (int32_t)j;
      J.off[n_jobs] = P.final_off;
    }
  } else {
    // rows: t_rows sums of t_cols consecutive elements; columns: t_cols sums of t_rows elements t_cols apart
    J.in[n_jobs] = in; J.cnt[n_jobs] = t_cols; J.stride[n_jobs] = P.final_cnt; J.bit[n_jobs] = -1; J.off[n_jobs] = 0;
    J.reps[n_jobs] = t_rows; J.rep_stride[n_jobs] = t_cols; J.elem_stride[n_jobs] = 1; J.limit[n_jobs] = P.final_cnt;
    ++n_jobs;
    J.in[n_jobs] = in; J.cnt[n_jobs] = t_rows; J.stride[n_jobs] = P.final_cnt; J.bit[n_jobs] = -1; J.off[n_jobs] = 0;
    J.reps[n_jobs] = t_cols; J.rep_stride[n_jobs] = 1; J.elem_stride[n_jobs] = t_cols; J.limit[n_jobs] = P.final_cnt;
    ++n_jobs;
  }
  const size_t lds = 256 * sizeof(typename BucketAcc<F>::type);
  XYZZ<F>* dst = W.sumtmp;
  for (uint32_t launch = 0;; ++launch) {
    const bool families = P.tail2d && launch == 0;  // (this launch leaves R and C behind: another one must follow)
    uint32_t left = 1;  // longest row of slice sums this launch leaves
    uint64_t o_dst = 0;
    for (uint32_t j = 0; j < n_jobs; ++j) {
      const uint32_t sl = (J.cnt[j] + MSM_TREE_SLICE - 1) / MSM_TREE_SLICE;
      J.first_block[j + 1] = J.first_block[j] + J.reps[j] * sl;
      if (sl > left) left = sl;
    }
    const bool last = left == 1 && !families;
    for (uint32_t j = 0; j < n_jobs; ++j) {
      const uint32_t sl = (J.cnt[j] + MSM_TREE_SLICE - 1) / MSM_TREE_SLICE;
      if (families && j >= n_levels) {            // rows -> rc[w][0 .. t_rows), columns -> rc[w][t_rows .. t_rows + t_cols)
        J.out[j] = W.rc + (j == n_levels ? 0 : t_rows);
        J.out_w[j] = t_rows + t_cols;
      } else if (last) {
        J.out[j] = W.wsums + j;
        J.out_w[j] = n_out;
      } else {
        J.out[j] = dst + o_dst;                   // WL x sl slice sums of this job
        J.out_w[j] = 1;
        o_dst += (uint64_t)WL * sl;
      }
    }
    J.n_jobs = n_jobs;
    hipLaunchKernelGGL(msm_tree_kernel<F>, dim3(J.first_block[n_jobs] * WL), dim3(256), lds, st, J);
    ZK_HIP(hipGetLastError());
    if (last) break;
    // next launch: plain sums of the rows of slice sums ...
    for (uint32_t j = 0; j < (families ? n_levels : n_jobs); ++j) {
      const uint32_t sl = (J.cnt[j] + MSM_TREE_SLICE - 1) / MSM_TREE_SLICE;
      J.in[j] = J.out[j];
      J.cnt[j] = J.stride[j] = sl;
      J.bit[j] = -1;
      plain(j);
    }
    if (families) {
      // ... and the bit decompositions of the column sums (weights c + off, 2^e) and of the row sums (weights r, 2^(cols_log + e))
      n_jobs = n_levels;
      for (uint32_t j = 0; j < P.final_bits; ++j, ++n_jobs) {
        plain(n_jobs);
        J.in[n_jobs] = W.rc + t_rows;
        J.cnt[n_jobs] = t_cols;
        J.stride[n_jobs] = t_rows + t_cols;
        J.bit[n_jobs] = (int32_t)j;
        J.off[n_jobs] = P.final_off;
      }
      for (uint32_t j = 0; j < P.row_bits; ++j, ++n_jobs) {
        plain(n_jobs);
        J.in[n_jobs] = W.rc;
        J.cnt[n_jobs] = t_rows;
        J.stride[n_jobs] = t_rows + t_cols;
        J.bit[n_jobs] = (int32_t)j;
      }
    }
    dst = dst == W.sumtmp ? W.sumtmp + (uint64_t)WL * P.tree_tmp : W.sumtmp;
  }
  return ZK_OK;
}

// ---- one base set's end: reduce, ONE copy back (window sums + error words), the Source errors, the host join
// d_bases / d_sc_first: table mode's error path rescans them.  last_set: the device-wide workspace lock is given up before the join.
template <class F>
int msm_finish_set(const MsmCall<F>& A, SmallWsLease& lease, std::unique_lock<std::mutex>& lk, const Affine<F>* d_bases, const uint32_t* d_sc_first,
                   Jacobian<F>* result, bool last_set, long long* err_index_out) {
  const MsmPlan& P = A.plan;
  const hipStream_t st = A.st;
  const size_t back_bytes = P.L.back_bytes();
  PinLease pin;
  if (int prc = pin_acquire(A.dev, back_bytes, &pin)) return prc;
  prof_begin(msm_slots().red, st);
  if (int rrc = launch_reduce(A)) return rrc;
  prof_end(msm_slots().red, st);
  if (msm_checkpoint(A, "reduce", P.chunks[0])) return (int)ZK_ERR_DEVICE;

  ZK_HIP(hipMemcpyAsync(pin.slot->p, A.ws.wsums, back_bytes, hipMemcpyDeviceToHost, st));
  // (parking on an event recorded in front of the reduction and polling the stream from there was measured in round 4: 1.790 against
  // 1.805 ms at 2^20, nothing at 2^12 .. 2^22 or for the prover's eight threads -- the runtime's own wait is not what a short call waits for)
  ZK_HIP(hipStreamSynchronize(st));
  const XYZZ<F>* h_wsums = reinterpret_cast<const XYZZ<F>*>(pin.slot->p);
  unsigned long long h_errs[2];
  std::memcpy(h_errs, (const char*)pin.slot->p + (back_bytes - 16), 16);
  lease.idle = true;
  const auto t_join0 = std::chrono::steady_clock::now();
  unsigned long long h_err = h_errs[0];
  if (P.tmode && h_err != ~0ull && h_errs[1] == ~0ull) {
    // (error path) the lowest identity BASE index, by exponent order: see msm_identity_scan_kernel
    lease.idle = false;
    ZK_HIP(hipMemsetAsync(A.ws.d_err, 0xff, 8, st));
    hipLaunchKernelGGL(msm_identity_scan_kernel<F>, dim3((unsigned)((A.n + 255) / 256)), dim3(256), 0, st, d_bases, d_sc_first, A.n, A.base_offset, A.d_density,
                       A.d_dprefix, A.ws.d_err);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(pin.slot->p, A.ws.d_err, 8, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));
    std::memcpy(&h_err, pin.slot->p, 8);
    lease.idle = true;
  }
  // the device is done with the workspace: let the next multiexp (another host thread -- the prover keeps 8 in
  // flight, prover.rs:250-298) start while this thread joins its partial sums
  if (last_set && lk.owns_lock()) lk.unlock();
  if (h_errs[1] != ~0ull) {
    *err_index_out = (long long)h_errs[1];
    return ZK_ERR_BAD_ARGS;
  }
  if (h_err != ~0ull) {
    *err_index_out = (long long)h_err;
    return ZK_ERR_UNEXPECTED_IDENTITY;
  }
  msm_join<F>(P, h_wsums, A.knobs.join_serial, result);
  if (A.knobs.trace_join)
    std::fprintf(stderr, "[mi355zk] msm n=%llu: host join of %u window sums: %.1f us\n", (unsigned long long)A.n, P.WL * P.n_out,
                 std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_join0).count());
  return (int)ZK_OK;
}

// Self-test tap (mi355zk_selftest_g1_msm_buckets_dev): a caller that sets this pointer for its thread gets, from a single-chunk call, the partition's
// index lists (first / last per bucket, the signed base indices) and the bucket records as the accumulation left them, copied to the host after the
// accumulate stage and before the reduction.  Nothing else reads it; the product's callers leave it null.
struct MsmBucketTap {
  uint32_t n_buckets = 0;
  std::vector<uint32_t> first, last, vals;
  std::vector<uint64_t> records;   // n_buckets records, sizeof(XYZZ<F>) / 8 words each
};
inline thread_local MsmBucketTap* g_msm_bucket_tap = nullptr;
template <class F>
int msm_tap_buckets(const MsmCall<F>& A, MsmBucketTap& T) {
  const uint32_t nb = A.plan.n_buckets;
  T.n_buckets = nb;
  T.first.resize(nb), T.last.resize(nb), T.records.resize((size_t)nb * sizeof(XYZZ<F>) / 8);
  ZK_HIP(hipMemcpyAsync(T.first.data(), A.ws.first, (size_t)nb * 4, hipMemcpyDeviceToHost, A.st));
  ZK_HIP(hipMemcpyAsync(T.last.data(), A.ws.last, (size_t)nb * 4, hipMemcpyDeviceToHost, A.st));
  ZK_HIP(hipMemcpyAsync(T.records.data(), A.ws.buckets, (size_t)nb * sizeof(XYZZ<F>), hipMemcpyDeviceToHost, A.st));
  ZK_HIP(hipStreamSynchronize(A.st));
  uint32_t top = 0;
  for (uint32_t b = 0; b < nb; ++b)
    if (T.last[b] > T.first[b] && T.last[b] > top) top = T.last[b];
  T.vals.resize(top);
  if (top) ZK_HIP(hipMemcpyAsync(T.vals.data(), A.ws.vals_b, (size_t)top * 4, hipMemcpyDeviceToHost, A.st));
  ZK_HIP(hipStreamSynchronize(A.st));
  return ZK_OK;
}

template <class F>
int msm_device(const Affine<F>* d_bases, uint64_t n_bases, uint64_t base_offset, const uint32_t* d_scalars, uint64_t n,
               const uint32_t* d_density, const uint32_t* d_dprefix, hipStream_t st, Jacobian<F>* out, long long* err_index_out,
               bool dense = false, const Affine<F>* d_bases2 = nullptr, Jacobian<F>* out2 = nullptr, uint32_t wgroups = 1,
               uint32_t wgroup = 0, bool scalars_mont = false, MsmChunks* chunks = nullptr, uint64_t table_stride = 0, uint32_t table_c = 0) {
  // table_stride != 0: TABLE MODE.  d_bases is a window table of the base vector -- table[w * table_stride + i] = 2^shift_w * bases[i]
  // for the windows of make_geom(table_c) (msm_table_build) -- so a digit of ANY window goes to the bucket of its value in ONE
  // bucket set shared by all windows: the W key planes the digit kernel writes are read as ONE array of W * kstride (digit, table
  // index) pairs, partitioned as a single window, accumulated into 2^(c-1) buckets and reduced once; the join is the window sum
  // itself.  What it buys: one window's reduction instead of W, and with it a wider window (fewer additions) on short calls.
  // wgroups > 1: only window group `wgroup` of `wgroups` equal groups is evaluated -- the partial  sum_{w in group} B^w T_w
  // of this point set; the partials of all groups (and of all point ranges) add up to the multiexp (shard.py).
  // dense == true: powersoftau's dense_multiexp contract (infinity bases add nothing, no Source errors);
  // d_bases2 != nullptr: a second base vector evaluated with the SAME exponents (merge_pairs), sharing the
  // digit extraction and the sorts.
  // chunks != nullptr: a STREAMED multiexp (the host-buffer entry point uploads the exponents while the kernels run).  The
  // exponents [cuts[c], cuts[c+1]) of chunk c are taken from the pointer chunks->acquire(c) hands out; geometry and bucket array
  // are those of the WHOLE call: every chunk runs digits -> partition -> accumulate into the SAME buckets (the first chunk
  // writes them, the others carry them on), and the reduction and the join run once.  d_scalars is ignored, d_density /
  // d_dprefix cover the whole call.
  *out = Jacobian<F>::zero();
  if (out2) *out2 = Jacobian<F>::zero();
  *err_index_out = -1;
  if (n == 0) return ZK_OK;
  if (n_bases > 0x7fffffffull || n > 0x7fffffffull) return ZK_ERR_BAD_ARGS;
  int dev = 0;
  ZK_HIP(hipGetDevice(&dev));
  struct Inflight {
    std::atomic<int>& c;
    explicit Inflight(std::atomic<int>& x) : c(x) { c.fetch_add(1, std::memory_order_relaxed); }
    ~Inflight() { c.fetch_sub(1, std::memory_order_relaxed); }
  } inflight(g_msm_inflight[dev & 15]);
  const MsmKnobs K = msm_knobs();
  MsmRequest R;
  R.group = (int)(sizeof(F) / sizeof(Fq));
  R.n = n;
  R.base_offset = base_offset;
  R.wgroups = wgroups;
  R.wgroup = wgroup;
  if (chunks) R.n_chunks = chunks->n_chunks, R.cuts = chunks->cuts;
  R.two_sets = d_bases2 != nullptr;
  R.table_stride = table_stride;
  R.table_c = table_c;
  const MsmPlan P = msm_plan(R, K);
  if (P.rc) return P.rc;

  int rc = part_configure<F>(dev);
  if (rc) return rc;
  // calls whose workspace is small lease a buffer of their own; the others share the device's, one at a time (msm_pools.hpp)
  Workspace& dev_ws = ws_of(dev);
  std::unique_lock<std::mutex> lk(dev_ws.mu, std::defer_lock);
  void* base = nullptr;
  SmallWsLease lease;
  if (P.L.total_bytes <= WS_SMALL) {
    rc = tws_acquire(dev, P.L.total_bytes, st, &lease, &base);
  } else {
    lk.lock();
    rc = dev_ws.buf.reserve(P.L.total_bytes);
    base = dev_ws.buf.p;
  }
  if (rc) return rc;
  const MsmCall<F> A{{P, K, R.group, dev, st, n, base_offset, table_stride, d_density, d_dprefix, scalars_mont}, MsmWs<F>((char*)base, P.L), dense};
  ZK_HIP(hipMemsetAsync(A.ws.d_err, 0xff, 16, st));
  lease.idle = false;

  const uint32_t* d_sc_first = d_scalars;
  for (uint32_t c = 0; c < (uint32_t)P.chunks.size(); ++c) {
    const ChunkPlan& C = P.chunks[c];
    const uint32_t* d_sc = d_scalars;
    if (chunks) {
      const void* p = nullptr;
      rc = chunks->acquire(c, st, &p);  // (makes `st` wait for the chunk's upload)
      if (rc) return rc;
      d_sc = (const uint32_t*)p;
    }
    d_sc_first = d_sc;  // (table mode runs a single chunk: its exponents, for the error path's rescan)
    rc = launch_digits(A, A.ws, C, d_sc);
    if (rc == ZK_OK && chunks) rc = chunks->digits_enqueued(c, st);  // the digit kernel is the only reader of the exponents
    if (rc == ZK_OK) rc = launch_partition(A, A.ws, C);
    if (rc == ZK_OK) rc = launch_accumulate(A, C, d_bases, c > 0);
    if (rc) return rc;
  }
  if (g_msm_bucket_tap) {
    if (P.chunks.size() != 1) return ZK_ERR_BAD_ARGS;
    if (int trc = msm_tap_buckets(A, *g_msm_bucket_tap)) return trc;
  }
  // bucket reduction, the copy back and the host join: once per base vector
  const bool two_sets = d_bases2 != nullptr && out2 != nullptr;
  rc = msm_finish_set(A, lease, lk, d_bases, d_sc_first, out, !two_sets, err_index_out);
  if (rc != ZK_OK || !two_sets) return rc;
  lease.idle = false;
  rc = launch_accumulate(A, P.chunks[0], d_bases2, false);
  if (rc) return rc;
  return msm_finish_set(A, lease, lk, d_bases, d_sc_first, out2, true, err_index_out);
}

// ---- A BATCH: n_vectors exponent vectors (vector v at d_scalars + v * scalar_stride * 8 words) over ONE base vector and ONE density map:
// out[v] / rcs[v] / err_index[v] are what msm_device returns for vector v alone.  The vectors are an axis in FRONT of the pipeline:
// the batched digit kernel writes vector v's WD key planes at v * WD, and the partition, the accumulation and the reduction run
// unchanged over WL = B' * WD bucket sets (MsmRequest::n_vectors) -- one launch sequence and one copy back for B' vectors.  A batch
// beyond the limits of one pass (msm_plan.hpp: msm_batch_split) runs several passes over consecutive vectors in the same workspace
// lease; every pass ends with ONE copy back and one join per vector (msm_join_batch), the last pass's after the workspace is given up.
// ERRORS: the pipeline's two error words stay call-wide.  A pass that sets either is discarded and its vectors are run by msm_device
// one by one, after the batch's device work: their return codes, error indices and points come from there (caller bugs, not a
// path to make fast).  The return value is that of the call as a whole (refused arguments, a device failure).
template <class F>
int msm_device_batch(const Affine<F>* d_bases, uint64_t n_bases, uint64_t base_offset, const uint32_t* d_scalars, uint64_t n, uint64_t scalar_stride,
                     uint32_t n_vectors, const uint32_t* d_density, const uint32_t* d_dprefix, hipStream_t st, Jacobian<F>* out, int* rcs,
                     long long* err_index_out, bool scalars_mont) {
  if (n_vectors == 0 || scalar_stride < n) return ZK_ERR_BAD_ARGS;
  for (uint32_t v = 0; v < n_vectors; ++v) out[v] = Jacobian<F>::zero(), rcs[v] = ZK_OK, err_index_out[v] = -1;
  if (n == 0) return ZK_OK;
  if (n_bases > 0x7fffffffull || n > 0x7fffffffull) return ZK_ERR_BAD_ARGS;
  auto single = [&](uint32_t v) {
    rcs[v] = msm_device<F>(d_bases, n_bases, base_offset, d_scalars + (uint64_t)v * scalar_stride * 8, n, d_density, d_dprefix, st, &out[v],
                           &err_index_out[v], false, nullptr, nullptr, 1, 0, scalars_mont);
  };
  const MsmKnobs K = msm_knobs();
  const int group = (int)(sizeof(F) / sizeof(Fq));
  const uint32_t per = n_vectors == 1 ? 1u : msm_batch_split(n, n_vectors, choose_geom(n, group, 1, K), group, K);
  if (per <= 1) {   // one vector, or a vector so long that two do not fit a pass: today's path
    if (n_vectors > 1 && K.fused_a) return ZK_ERR_BAD_ARGS;   // (as launch_digits answers a batch under the fused pass A)
    for (uint32_t v = 0; v < n_vectors; ++v) single(v);
    return ZK_OK;
  }
  int dev = 0;
  ZK_HIP(hipGetDevice(&dev));
  // the plans: full passes of `per` vectors and, when per does not divide the batch, a shorter last one
  MsmRequest R;
  R.group = group;
  R.n = n;
  R.base_offset = base_offset;
  R.n_vectors = per;
  const MsmPlan P_full = msm_plan(R, K);
  if (P_full.rc) return P_full.rc;
  const uint32_t n_pass = msm_batch_passes(n_vectors, per), last_cnt = msm_batch_pass(n_vectors, per, n_pass - 1).count;
  MsmPlan P_last;
  if (last_cnt != per && last_cnt > 1) {
    R.n_vectors = last_cnt;
    P_last = msm_plan(R, K);
    if (P_last.rc) return P_last.rc;
  }
  const bool last_single = last_cnt == 1;   // a lone last vector takes the single call
  const uint32_t n_batched = last_single ? n_pass - 1 : n_pass;
  auto plan_of = [&](uint32_t p) -> const MsmPlan& { return (p + 1 == n_pass && last_cnt != per) ? P_last : P_full; };
  std::vector<uint8_t> redo(n_vectors, 0);
  {
    struct Inflight {
      std::atomic<int>& c;
      explicit Inflight(std::atomic<int>& x) : c(x) { c.fetch_add(1, std::memory_order_relaxed); }
      ~Inflight() { c.fetch_sub(1, std::memory_order_relaxed); }
    } inflight(g_msm_inflight[dev & 15]);
    int rc = part_configure<F>(dev);
    if (rc) return rc;
    size_t ws_bytes = 0, pin_bytes = 0;
    for (uint32_t p = 0; p < n_batched; ++p) {
      ws_bytes = std::max(ws_bytes, plan_of(p).L.total_bytes);
      pin_bytes = std::max(pin_bytes, plan_of(p).L.back_bytes());
    }
    PinLease pin;
    if (int prc = pin_acquire(dev, pin_bytes, &pin)) return prc;
    Workspace& dev_ws = ws_of(dev);
    std::unique_lock<std::mutex> lk(dev_ws.mu, std::defer_lock);
    void* base = nullptr;
    SmallWsLease lease;
    if (ws_bytes <= WS_SMALL) {
      rc = tws_acquire(dev, ws_bytes, st, &lease, &base);
    } else {
      lk.lock();
      rc = dev_ws.buf.reserve(ws_bytes);
      base = dev_ws.buf.p;
    }
    if (rc) return rc;
    double join_us = 0;
    for (uint32_t p = 0; p < n_batched; ++p) {
      const MsmPlan& P = plan_of(p);
      const MsmBatchPass pass = msm_batch_pass(n_vectors, per, p);
      const MsmCall<F> A{{P, K, group, dev, st, n, base_offset, 0, d_density, d_dprefix, scalars_mont, scalar_stride}, MsmWs<F>((char*)base, P.L), false};
      const ChunkPlan& C = P.chunks[0];
      lease.idle = false;
      ZK_HIP(hipMemsetAsync(A.ws.d_err, 0xff, 16, st));
      rc = launch_digits(A, A.ws, C, d_scalars + (uint64_t)pass.first * scalar_stride * 8);
      if (rc == ZK_OK) rc = launch_partition(A, A.ws, C);
      if (rc == ZK_OK) rc = launch_accumulate(A, C, d_bases, false);
      if (rc) return rc;
      prof_begin(msm_slots().red, st);
      if (int rrc = launch_reduce(A)) return rrc;
      prof_end(msm_slots().red, st);
      if (msm_checkpoint(A, "reduce", C)) return (int)ZK_ERR_DEVICE;
      // ONE copy back per pass: the window sums of all its vectors and the two error words
      ZK_HIP(hipMemcpyAsync(pin.slot->p, A.ws.wsums, P.L.back_bytes(), hipMemcpyDeviceToHost, st));
      ZK_HIP(hipStreamSynchronize(st));
      lease.idle = true;
      if (p + 1 == n_batched) {   // the device is done with the workspace: the last joins are host work beside the next call
        if (lk.owns_lock()) lk.unlock();
        lease.release();
      }
      unsigned long long h_errs[2];
      std::memcpy(h_errs, (const char*)pin.slot->p + (P.L.back_bytes() - 16), 16);
      if (h_errs[0] != ~0ull || h_errs[1] != ~0ull) {   // some vector of the pass has a Source error or a non-canonical exponent: the single calls say which
        for (uint32_t v = 0; v < pass.count; ++v) redo[pass.first + v] = 1;
        continue;
      }
      const auto t_join0 = std::chrono::steady_clock::now();
      msm_join_batch<F>(P, reinterpret_cast<const XYZZ<F>*>(pin.slot->p), pass.count, K.join_serial, out + pass.first);
      join_us += std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_join0).count();
    }
    if (K.trace_join)
      std::fprintf(stderr, "[mi355zk] msm batch n=%llu x %u: host joins of %u passes: %.1f us\n", (unsigned long long)n, n_vectors, n_batched, join_us);
  }
  if (last_single) redo[n_vectors - 1] = 1;
  for (uint32_t v = 0; v < n_vectors; ++v)
    if (redo[v]) single(v);
  return ZK_OK;
}

// ------------------------------------------------------------------------------------------------
// Segmented sum of affine points: out[r] = sum of points[row_ptr[r] .. row_ptr[r+1]), normalised to affine.
// This is the bucket accumulation above with the rows of a CSR matrix as the "buckets" (size-ordered lanes,
// segment-parallel path for long rows), used by the QAP evaluation of phase2/src/parameters.rs:225-294
// (per variable: sum of coeff * Lagrange-basis point, then batch_normalization).
template <class F>
int segsum_device(const Affine<F>* d_points, uint64_t nnz, const uint32_t* d_row_ptr, uint32_t n_rows, hipStream_t st, Affine<F>* d_out) {
  if (n_rows == 0) return ZK_OK;
  if (nnz >= 0x7fffffffull) return ZK_ERR_BAD_ARGS;
  int dev = 0;
  ZK_HIP(hipGetDevice(&dev));
  const uint32_t* first = d_row_ptr;
  const uint32_t* last = d_row_ptr + 1;
  const uint64_t mean_len = nnz / n_rows + 1;
  const uint32_t heavy = (uint32_t)(mean_len * 8 + 1024 > 0xffffffffull ? 0xffffffffull : mean_len * 8 + 1024);
  uint32_t hb = n_rows < MSM_HEAVY_BLOCKS ? n_rows : MSM_HEAVY_BLOCKS;
  if ((uint64_t)hb > nnz / heavy + 1) hb = (uint32_t)(nnz / heavy + 1);
  const uint32_t max_items = (uint32_t)(nnz / MSM_HEAVY_SEG) + hb;
  size_t off = 0;
  auto take = [&](size_t bytes) { size_t o = off; off += align_up(bytes); return o; };
  size_t o_vals = take((size_t)(nnz ? nnz : 1) * 4);
  size_t o_hist = take(MSM_SIZE_BINS * 4), o_sizes_b = take((size_t)n_rows * 4), o_order = take((size_t)n_rows * 4);
  size_t o_item_off = take((size_t)(hb + 2) * 4);
  size_t o_seg = take((size_t)max_items * sizeof(XYZZ<F>));
  size_t o_buckets = take((size_t)n_rows * sizeof(XYZZ<F>));
  Workspace& dev_ws = ws_of(dev);
  std::lock_guard<std::mutex> lk(dev_ws.mu);
  int rc = dev_ws.buf.reserve(off);
  if (rc) return rc;
  char* ws = (char*)dev_ws.buf.p;
  uint32_t* vals = (uint32_t*)(ws + o_vals);
  uint32_t* size_hist = (uint32_t*)(ws + o_hist);
  uint32_t* sizes_b = (uint32_t*)(ws + o_sizes_b);
  uint32_t* order = (uint32_t*)(ws + o_order);
  uint32_t* item_off = (uint32_t*)(ws + o_item_off);
  XYZZ<F>* seg_sums = (XYZZ<F>*)(ws + o_seg);
  XYZZ<F>* buckets = (XYZZ<F>*)(ws + o_buckets);
  if (nnz) launch_iota(st, vals, (uint32_t)nnz);
  ZK_HIP(hipMemsetAsync(size_hist, 0, MSM_SIZE_BINS * 4, st));
  msm_order_by_size(first, last, n_rows, size_hist, order, sizes_b, st);
  ZK_HIP(hipGetLastError());
  // (rows are dense sums: the identity adds nothing, no error word; nothing is carried)
  rc = launch_heavy(st, d_points, vals, first, last, order, sizes_b, item_off, seg_sums, buckets, (unsigned long long*)nullptr,
                    HeavyParams{hb, heavy, MSM_HEAVY_SEG, max_items < 16384 ? max_items : 16384, 1, 0});
  if (rc) return rc;
  hipLaunchKernelGGL((msm_accumulate_kernel<F, false, false>), dim3((n_rows + 255) / 256), dim3(256), 0, st, d_points, vals, first, last, order, heavy, hb,
                     n_rows, buckets, 1, (unsigned long long*)nullptr);
  hipLaunchKernelGGL(msm_to_affine_kernel<F>, dim3((n_rows + 255) / 256), dim3(256), 0, st, buckets, d_out, n_rows);
  ZK_HIP(hipGetLastError());
  ZK_HIP(hipStreamSynchronize(st));  // the workspace is shared: finish before releasing the lock
  return ZK_OK;
}

}  // namespace

}  // namespace zk
