// The pairing on the device (include/mi355zk.h; the arithmetic: pairing.hpp): what same_ratio (powersoftau/src/utils.rs:151-159), the
// per-contribution checks of MPCParameters::verify (phase2/src/parameters.rs:529-659) and groth16 verify_proof (bellman/src/groth16/
// verifier.rs:36-67) end in, in its batched form -- many independent pairing products at once.  Three stages on the caller's stream:
//   1. pairing_miller_kernel      one lane per pair: the Miller value, 384 B, into a workspace
//   2. pairing_product_kernel     the product of each group's values (groups in CSR form), in place: a lane multiplies one run of at most 64
//                                 values into the run's first slot, and the pass repeats over the run heads until every group has one value
//   3. pairing_final_exp_kernel   one lane per group: the final exponentiation of the group's value, or of one for an empty group
// No communication between lanes anywhere.  The workspace is one stream-ordered allocation per call (hipMallocAsync / hipFreeAsync).
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/mi355zk.h"
#include "pairing.hpp"

#include "api_internal.hpp"

namespace zk {
namespace {

constexpr unsigned PAIRING_BLOCK = 64;   // one wave per block: a launch of a few thousand lanes spreads over as many CUs as it has waves
constexpr uint64_t PAIRING_RUN = 64;     // values one lane multiplies in a row in one pass

__global__ void __launch_bounds__(PAIRING_BLOCK) pairing_miller_kernel(Fq12* __restrict__ out, const Affine<Fq>* __restrict__ g1,
                                                                       const Affine<Fq2>* __restrict__ g2, uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * PAIRING_BLOCK + threadIdx.x;
  if (i >= n) return;
  const Affine<Fq> p = g1[i];
  const Affine<Fq2> q = g2[i];
  Fq12 f;
  pairing_miller_loop(f, p, q);
  out[i] = f;
}

// One pass of the segmented product.  Before the pass the values of group g are w[begin + k * stride], k < ceil(L / stride), with
// [begin, begin + L) the group's range; after it they are w[begin + k * run], run = 64 * stride: the lane of run m multiplies the (at most
// 64) values of [begin + m * run, begin + (m + 1) * run) into the first of them.  Runs are disjoint, so the pass works in place.
// Lanes are numbered without a prefix sum over the groups: group g owns the slots from slot(g) = begin / run + g, and
// slot(g + 1) - slot(g) >= L / run + 1 covers its ceil(L / run) runs; a lane finds its group by bisection over slot().
// group_ptr is the caller's and is NOT trusted: entries are clamped to n, so a pointer array that is not nondecreasing gives unspecified
// values and never an access outside w[0, n).
__device__ __forceinline__ uint64_t group_begin(const uint32_t* __restrict__ group_ptr, uint64_t g, uint64_t n) {
  const uint64_t p = group_ptr[g];
  return p < n ? p : n;
}
__global__ void __launch_bounds__(PAIRING_BLOCK) pairing_product_kernel(Fq12* __restrict__ w, const uint32_t* __restrict__ group_ptr,
                                                                        uint64_t n_groups, uint64_t n, uint64_t stride, uint64_t slots) {
  const uint64_t t = (uint64_t)blockIdx.x * PAIRING_BLOCK + threadIdx.x;
  if (t >= slots) return;
  const uint64_t run = stride * PAIRING_RUN;
  uint64_t lo = 0, hi = n_groups - 1;                       // the last group whose first slot is <= t
  while (lo < hi) {
    const uint64_t mid = lo + (hi - lo + 1) / 2;
    if (group_begin(group_ptr, mid, n) / run + mid <= t) lo = mid;
    else hi = mid - 1;
  }
  const uint64_t begin = group_begin(group_ptr, lo, n), end = group_begin(group_ptr, lo + 1, n), slot = begin / run + lo;
  if (slot > t || end <= begin) return;
  const uint64_t first = (t - slot) * run, len = end - begin;   // (t - slot) < slots <= n / run + n_groups: no overflow
  if (first >= len) return;
  const uint64_t span = len - first < run ? len - first : run;
  const uint64_t count = (span + stride - 1) / stride;          // <= 64
  if (count <= 1) return;
  Fq12* head = w + begin + first;                               // head + k * stride < w + end <= w + n for k < count
  Fq12 acc = *head;
#pragma unroll 1
  for (uint64_t k = 1; k < count; ++k) {
    const Fq12 v = head[k * stride];
    fq12_mul(acc, acc, v);
  }
  *head = acc;
}

// group_ptr == nullptr: group g is the single value w[g]
__global__ void __launch_bounds__(PAIRING_BLOCK) pairing_final_exp_kernel(Fq12* __restrict__ out, const Fq12* __restrict__ w,
                                                                          const uint32_t* __restrict__ group_ptr, uint64_t n_groups, uint64_t n) {
  const uint64_t g = (uint64_t)blockIdx.x * PAIRING_BLOCK + threadIdx.x;
  if (g >= n_groups) return;
  Fq12 f = fq12_one();
  if (group_ptr) {
    const uint64_t begin = group_begin(group_ptr, g, n), end = group_begin(group_ptr, g + 1, n);
    if (end > begin) f = w[begin];
  } else {
    f = w[g];
  }
  Fq12 o;
  pairing_final_exponentiation(o, f);
  out[g] = o;
}

// flags[i] = a[i] == (b ? b[i] : one), bytes
__global__ void __launch_bounds__(256) gt_eq_kernel(uint8_t* __restrict__ flags, const uint32_t* __restrict__ a, const uint32_t* __restrict__ b,
                                                    uint64_t n) {
  const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  constexpr int WORDS = (int)(sizeof(Fq12) / 4);
  const uint32_t* x = a + i * WORDS;
  uint32_t diff = 0;
  if (b) {
    const uint32_t* y = b + i * WORDS;
    for (int k = 0; k < WORDS; ++k) diff |= x[k] ^ y[k];
  } else {
#pragma unroll
    for (int k = 0; k < 8; ++k) diff |= x[k] ^ FqParams::R[k];   // one: c0.c0.c0 = R, eleven zeros
    for (int k = 8; k < WORDS; ++k) diff |= x[k];
  }
  flags[i] = diff == 0 ? 1 : 0;
}

inline unsigned blocks_of(uint64_t lanes, unsigned block) { return (unsigned)((lanes + block - 1) / block); }

int pairing_product_dev(void* d_out, const void* d_g1, const void* d_g2, size_t n_pairs, const uint32_t* d_group_ptr, size_t n_groups, void* stream) {
  constexpr size_t LIMIT = (size_t)1 << 31;
  if (n_pairs >= LIMIT || n_groups >= LIMIT) return ZK_ERR_BAD_ARGS;
  if (n_pairs && (!d_g1 || !d_g2)) return ZK_ERR_BAD_ARGS;
  if (n_groups && !d_out) return ZK_ERR_BAD_ARGS;
  if (!d_group_ptr && n_groups != n_pairs) return ZK_ERR_BAD_ARGS;
  if (n_groups == 0) return ZK_OK;
  static const int slot_miller = prof_slot("pairing_miller"), slot_product = prof_slot("pairing_product"),
                   slot_final = prof_slot("pairing_final_exp");
  hipStream_t st = (hipStream_t)stream;
  Fq12* w = nullptr;
  if (n_pairs) {
    void* p = nullptr;
    ZK_HIP(hipMallocAsync(&p, n_pairs * sizeof(Fq12), st));
    w = (Fq12*)p;
  }
  int rc = ZK_OK;
  auto launched = [&]() {
    if (hipGetLastError() != hipSuccess) rc = ZK_ERR_DEVICE;
    return rc == ZK_OK;
  };
  if (n_pairs) {
    prof_begin(slot_miller, st);
    hipLaunchKernelGGL(pairing_miller_kernel, dim3(blocks_of(n_pairs, PAIRING_BLOCK)), dim3(PAIRING_BLOCK), 0, st, w, (const Affine<Fq>*)d_g1,
                       (const Affine<Fq2>*)d_g2, (uint64_t)n_pairs);
    prof_end(slot_miller, st);
  }
  if (launched() && d_group_ptr && n_pairs > 1) {
    // the caller's pointers are on the device: the longest group is only known to be at most n_pairs long
    prof_begin(slot_product, st);
    for (uint64_t stride = 1; stride < n_pairs && launched(); stride *= PAIRING_RUN) {
      const uint64_t slots = n_pairs / (stride * PAIRING_RUN) + n_groups;
      hipLaunchKernelGGL(pairing_product_kernel, dim3(blocks_of(slots, PAIRING_BLOCK)), dim3(PAIRING_BLOCK), 0, st, w, d_group_ptr,
                         (uint64_t)n_groups, (uint64_t)n_pairs, stride, slots);
    }
    prof_end(slot_product, st);
  }
  if (launched()) {
    prof_begin(slot_final, st);
    hipLaunchKernelGGL(pairing_final_exp_kernel, dim3(blocks_of(n_groups, PAIRING_BLOCK)), dim3(PAIRING_BLOCK), 0, st, (Fq12*)d_out, w,
                       d_group_ptr, (uint64_t)n_groups, (uint64_t)n_pairs);
    prof_end(slot_final, st);
    launched();
  }
  if (w && hipFreeAsync(w, st) != hipSuccess && rc == ZK_OK) rc = ZK_ERR_DEVICE;
  return rc;
}

int gt_eq_dev(uint8_t* d_flags, const void* d_a, const void* d_b, bool against_one, size_t n, void* stream) {
  if (n == 0) return ZK_OK;
  if (!d_flags || !d_a || (!against_one && !d_b) || n >= ((size_t)1 << 31)) return ZK_ERR_BAD_ARGS;
  hipLaunchKernelGGL(gt_eq_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, (hipStream_t)stream, d_flags, (const uint32_t*)d_a,
                     against_one ? nullptr : (const uint32_t*)d_b, (uint64_t)n);
  ZK_HIP(hipGetLastError());
  return ZK_OK;
}

int pairing_product_host(uint64_t* gt_out, const uint64_t* g1, const uint64_t* g2, size_t n) {
  if (!gt_out || n >= ((size_t)1 << 31) || (n && (!g1 || !g2))) return ZK_ERR_BAD_ARGS;
  Fq12 acc = fq12_one();
  for (size_t i = 0; i < n; ++i) {
    Affine<Fq> p;
    Affine<Fq2> q;
    std::memcpy(&p, g1 + 8 * i, sizeof p);
    std::memcpy(&q, g2 + 16 * i, sizeof q);
    Fq12 f;
    pairing_miller_loop(f, p, q);
    fq12_mul(acc, acc, f);
  }
  Fq12 out;
  pairing_final_exponentiation(out, acc);
  std::memcpy(gt_out, &out, sizeof out);
  return ZK_OK;
}

// one primitive of pairing.hpp on the host (the op list: include/mi355zk.h); the word counts are part of the contract
int selftest_pairing_op(int op, const uint64_t* in, size_t in_words, uint64_t* out, size_t out_words) {
  if (!in || !out) return ZK_ERR_BAD_ARGS;
  constexpr size_t W2 = 8, W6 = 24, W12 = 48;
  auto shape = [&](size_t want_in, size_t want_out) { return in_words == want_in && out_words == want_out; };
  Fq6 a6, b6;
  Fq12 a12, b12;
  Fq2 s[3];
  switch (op) {
    case MI355ZK_PAIRING_OP_FQ6_MUL:
      if (!shape(2 * W6, W6)) return ZK_ERR_BAD_ARGS;
      std::memcpy(&a6, in, sizeof a6);
      std::memcpy(&b6, in + W6, sizeof b6);
      fq6_mul(a6, a6, b6);
      std::memcpy(out, &a6, sizeof a6);
      return ZK_OK;
    case MI355ZK_PAIRING_OP_FQ6_INV:
      if (!shape(W6, W6)) return ZK_ERR_BAD_ARGS;
      std::memcpy(&a6, in, sizeof a6);
      fq6_inv(a6, a6);
      std::memcpy(out, &a6, sizeof a6);
      return ZK_OK;
    case MI355ZK_PAIRING_OP_FQ6_MUL_BY_01:
    case MI355ZK_PAIRING_OP_FQ6_MUL_BY_1: {
      const size_t k = op == MI355ZK_PAIRING_OP_FQ6_MUL_BY_01 ? 2 : 1;
      if (!shape(W6 + k * W2, W6)) return ZK_ERR_BAD_ARGS;
      std::memcpy(&a6, in, sizeof a6);
      std::memcpy(s, in + W6, k * sizeof(Fq2));
      if (k == 2) fq6_mul_by_01(a6, a6, s[0], s[1]);
      else fq6_mul_by_1(a6, a6, s[0]);
      std::memcpy(out, &a6, sizeof a6);
      return ZK_OK;
    }
    case MI355ZK_PAIRING_OP_FQ12_MUL:
      if (!shape(2 * W12, W12)) return ZK_ERR_BAD_ARGS;
      std::memcpy(&a12, in, sizeof a12);
      std::memcpy(&b12, in + W12, sizeof b12);
      fq12_mul(a12, a12, b12);
      std::memcpy(out, &a12, sizeof a12);
      return ZK_OK;
    case MI355ZK_PAIRING_OP_FQ12_MUL_BY_034:
      if (!shape(W12 + 3 * W2, W12)) return ZK_ERR_BAD_ARGS;
      std::memcpy(&a12, in, sizeof a12);
      std::memcpy(s, in + W12, 3 * sizeof(Fq2));
      fq12_mul_by_034(a12, s[0], s[1], s[2]);
      std::memcpy(out, &a12, sizeof a12);
      return ZK_OK;
    case MI355ZK_PAIRING_OP_FQ12_SQR:
    case MI355ZK_PAIRING_OP_FQ12_INV:
    case MI355ZK_PAIRING_OP_FQ12_CONJUGATE:
    case MI355ZK_PAIRING_OP_FQ12_FROBENIUS_1:
    case MI355ZK_PAIRING_OP_FQ12_FROBENIUS_2:
    case MI355ZK_PAIRING_OP_FQ12_FROBENIUS_3:
    case MI355ZK_PAIRING_OP_FINAL_EXPONENTIATION:
      if (!shape(W12, W12)) return ZK_ERR_BAD_ARGS;
      std::memcpy(&a12, in, sizeof a12);
      if (op == MI355ZK_PAIRING_OP_FQ12_SQR) fq12_sqr(b12, a12);
      else if (op == MI355ZK_PAIRING_OP_FQ12_INV) fq12_inv(b12, a12);
      else if (op == MI355ZK_PAIRING_OP_FQ12_CONJUGATE) fq12_conjugate(b12, a12);
      else if (op == MI355ZK_PAIRING_OP_FINAL_EXPONENTIATION) pairing_final_exponentiation(b12, a12);
      else fq12_frobenius_map(b12, a12, op - MI355ZK_PAIRING_OP_FQ12_FROBENIUS_1 + 1);
      std::memcpy(out, &b12, sizeof b12);
      return ZK_OK;
    default:
      return ZK_ERR_BAD_ARGS;
  }
}

}  // namespace
}  // namespace zk

extern "C" {

int mi355zk_bn254_pairing_product_dev(void* d_gt_out, const void* d_g1_affine, const void* d_g2_affine, size_t n_pairs, const uint32_t* d_group_ptr,
                                      size_t n_groups, void* stream) {
  return zk::abi_guard([&]() -> int { return zk::pairing_product_dev(d_gt_out, d_g1_affine, d_g2_affine, n_pairs, d_group_ptr, n_groups, stream); });
}
int mi355zk_bn254_gt_is_one_dev(uint8_t* d_flags, const void* d_gt, size_t n, void* stream) {
  return zk::abi_guard([&]() -> int { return zk::gt_eq_dev(d_flags, d_gt, nullptr, true, n, stream); });
}
int mi355zk_bn254_gt_eq_dev(uint8_t* d_flags, const void* d_gt_a, const void* d_gt_b, size_t n, void* stream) {
  return zk::abi_guard([&]() -> int { return zk::gt_eq_dev(d_flags, d_gt_a, d_gt_b, false, n, stream); });
}
int mi355zk_bn254_pairing_product(uint64_t gt_out[48], const uint64_t* g1_affine, const uint64_t* g2_affine, size_t n_pairs) {
  return zk::abi_guard([&]() -> int { return zk::pairing_product_host(gt_out, g1_affine, g2_affine, n_pairs); });
}
int mi355zk_selftest_pairing_op(int op, const uint64_t* in, size_t in_words, uint64_t* out, size_t out_words) {
  return zk::abi_guard([&]() -> int { return zk::selftest_pairing_op(op, in, in_words, out, out_words); });
}

}  // extern "C"
