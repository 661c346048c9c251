#pragma once
// Interface of msm_partition.hip: the stages of the Pippenger pipeline that do not depend on the curve group -- digits, partition,
// the size order of the buckets, the plan of the heavy path -- compiled ONCE and called by both instantiations of the host driver
// (msm_host.hpp, included by msm_g1.hip and by msm_g2.hip).  Nothing here names a field or a curve type.
#include <hip/hip_runtime.h>

#include <atomic>
#include <type_traits>

#include "device_util.hpp"
#include "msm_plan.hpp"

namespace zk {

// multiexps inside msm_device per device, G1 and G2 together: a call that has the device to itself may take every register of a SIMD
// (the two-wave G2 accumulation); one of the prover's eight concurrent calls leaves room for the others
extern std::atomic<int> g_msm_inflight[16];

// the untyped part of a call's workspace as pointers (MsmLayout's offsets over the leased buffer); MsmWs<F> (msm_host.hpp) adds the records
struct MsmPartWs {
  uint32_t *keys, *vals_b;  // (the index lists alias the keys: MsmLayout)
  uint2* pairs;
  uint16_t* tile_hist;
  uint32_t *tile_off, *csum, *col_total, *bin_start, *out_start, *gcnt, *gcur, *big_col, *big_seg;
  BigPlan* big_plan;
  uint32_t *first, *last, *size_hist, *sizes_b, *order, *item_off;
  unsigned long long* d_err;
  template <class T>
  static void at(char* ws, T*& p, size_t off) { p = reinterpret_cast<T*>(ws + off); }
  MsmPartWs(char* ws, const MsmLayout& L) {
    at(ws, keys, L.keys), at(ws, vals_b, L.keys), at(ws, pairs, L.pairs), at(ws, tile_hist, L.tile_hist), at(ws, tile_off, L.tile_off), at(ws, csum, L.csum);
    at(ws, col_total, L.total), at(ws, bin_start, L.bin_start), at(ws, out_start, L.out_start), at(ws, gcnt, L.gcnt), at(ws, gcur, L.gcur);
    at(ws, big_col, L.big_col), at(ws, big_seg, L.big_seg), at(ws, big_plan, L.big_plan), at(ws, first, L.first), at(ws, last, L.last);
    at(ws, size_hist, L.hist), at(ws, sizes_b, L.sizes_b), at(ws, order, L.ids_b), at(ws, item_off, L.item_off), at(ws, d_err, L.err);
  }
};

// what the group-independent launch stages of one msm_device call see; MsmCall<F> (msm_host.hpp) derives from it
struct MsmPartCall {
  const MsmPlan& plan;
  const MsmKnobs& knobs;
  int group;  // 1: G1, 2: G2 (msm_checkpoint's debug line)
  int dev;
  hipStream_t st;
  uint64_t n, base_offset, table_stride;
  const uint32_t *d_density, *d_dprefix;  // cover the whole call
  bool scalars_mont;
  uint64_t scalar_stride = 0;  // a batch (plan.n_vectors > 1): exponents between vector v and vector v + 1
};

struct MsmSlots { int digits, scan, scatter, bucket, sort, acc, heavy, red; };
inline const MsmSlots& msm_slots() {
  static const MsmSlots s{prof_slot("msm_digits"), prof_slot("msm_part_scan"), prof_slot("msm_scatter"), prof_slot("msm_bucket"),
                          prof_slot("msm_sort"), prof_slot("msm_accumulate"), prof_slot("msm_accumulate_heavy"), prof_slot("msm_reduce")};
  return s;
}

// MsmKnobs::debug: synchronise and report after a stage; non-zero if the stage failed
int msm_checkpoint(const MsmPartCall& A, const char* what, const ChunkPlan& C);

// the partition kernels use up to the whole 160 KiB of LDS (dynamic): raises their limit once per device, whichever group calls first; a
// failure is remembered and returned to every later call on that device
int part_configure(int dev);

// ---- digits of one chunk: window-major keys and the tile histograms
int launch_digits(const MsmPartCall& A, const MsmPartWs& W, const ChunkPlan& C, const uint32_t* d_sc);
// ---- partition of one chunk: index lists per (window, bucket) in vals_b, bounds first[] / last[], size order
int launch_partition(const MsmPartCall& A, const MsmPartWs& W, const ChunkPlan& C);
// order[] = the buckets by descending size bin, sizes_sorted[] their sizes.  hist: MSM_SIZE_BINS words, zeroed by the caller
void msm_order_by_size(const uint32_t* first, const uint32_t* last, uint32_t n_buckets, uint32_t* hist, uint32_t* order, uint32_t* sizes_sorted,
                       hipStream_t st);
// msm_heavy_plan_kernel (one workgroup): item_off (hb + 2 words) for the buckets longer than `heavy` among the hb leading entries of the size order
void launch_heavy_plan(hipStream_t st, const uint32_t* sizes_sorted, uint32_t hb, uint32_t heavy, uint32_t seg, uint32_t* item_off);
// v[i] = i for i < n (segsum_device: the index list of the identity order); n > 0
void launch_iota(hipStream_t st, uint32_t* v, uint32_t n);

}  // namespace zk
