// out[i] = in[i + shift] - in[i] on raw affine G1 records (include/mi355zk.h: mi355zk_bn254_g1_shifted_difference_dev): the H bases of
// powersoftau/src/bin/prepare_phase2.rs:137-147, h[i] = tau_g1[i + m] - tau_g1[i], without the index and coefficient arrays that the sparse
// point product needs to say "subtract your neighbour m places up" (72 B per output; 9 GiB of them at m = 2^27).
//
// One affine chord (or tangent) per output: lambda = (y2 + y1) / (x2 - x1), x3 = lambda^2 - x1 - x2, y3 = lambda (x2 - x3) - y2 for
// in[i] = (x1, y1), in[i + shift] = (x2, y2).  A lane owns K = MI355ZK_SHIFTED_DIFFERENCE_K consecutive outputs and inverts the product of
// their K denominators once (Montgomery's trick, the scheme of batch_normalize_kernel in scalar_mul.hip): per output 3 multiplications for
// the trick and 2M + 1S for the chord, next to 1 / K of an inversion (~380 multiplications).  An output that needs no inversion -- an
// operand or the result at infinity -- contributes one to the product, never zero.
//
// Access: a lane reads its K records of each operand one after the other, so the lanes of a wave are 64 K B = 1 KiB apart in each load.  Every
// lane still consumes whole 64-B records with four 16-B loads, and the inversion keeps the kernel on the VALU; a lane-per-output load with
// the inversion shared through LDS has not been measured against it.
#include <hip/hip_runtime.h>

#include <cstring>

#include "../../include/mi355zk.h"
#include "curve.hpp"
#include "fieldu.hpp"   // for_limbs
#include "device_util.hpp"
#include "api_internal.hpp"

namespace zk {
namespace {

constexpr int DIFF_K = MI355ZK_SHIFTED_DIFFERENCE_K;

ZK_HD G1Affine diff_load(const G1Affine* p) {
#if defined(__HIP_DEVICE_COMPILE__)
  union { uint4 q[4]; G1Affine a; } u;
  const uint4* s = reinterpret_cast<const uint4*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) u.q[i] = s[i];
  return u.a;
#else
  G1Affine r;
  std::memcpy(&r, p, sizeof r);
  return r;
#endif
}

ZK_HD void diff_store(G1Affine* p, const G1Affine& v) {
#if defined(__HIP_DEVICE_COMPILE__)
  union { uint4 q[4]; G1Affine a; } u;
  u.a = v;
  uint4* d = reinterpret_cast<uint4*>(p);
#pragma unroll
  for (int i = 0; i < 4; ++i) d[i] = u.q[i];
#else
  std::memcpy(p, &v, sizeof v);
#endif
}

// b - a needs the slope num / den: true, with the chord through b and -a, or -- when b == -a -- the tangent at b (its x equals a's, so one
// formula finishes both).  false: no inversion; the result is then `direct` (b, -a or infinity).
ZK_HD bool diff_slope(const G1Affine& a, const G1Affine& b, Fq& num, Fq& den, G1Affine& direct) {
  if (a.is_zero()) { direct = b; return false; }
  if (b.is_zero()) { direct = G1Affine{a.x, neg(a.y)}; return false; }
  if (a.x != b.x) {
    num = add(b.y, a.y);
    den = sub(b.x, a.x);
    return true;
  }
  if (a.y == b.y) { direct = G1Affine{Fq::zero(), Fq::zero()}; return false; }   // b == a (y == 0 included: a point of order two is its own inverse)
  const Fq xx = sqr(b.x);
  num = add(dbl(xx), xx);
  den = dbl(b.y);
  return true;
}

// outputs i0 .. i0 + K - 1 (those below n_out): two passes over the operands, the prefix products of the denominators between them
template <int K>
ZK_HD void shifted_difference_lane(G1Affine* out, const G1Affine* in, uint64_t i0, uint64_t shift, uint64_t n_out) {
  Fq pre[K];
  Fq run = Fq::one();
  // for_limbs: the index is a compile-time constant, which keeps pre[] in registers
  for_limbs<K>([&](auto kc) {
    constexpr int k = decltype(kc)::value;
    pre[k] = run;
    if (i0 + k < n_out) {
      Fq num, den;
      G1Affine direct;
      if (diff_slope(diff_load(in + i0 + k), diff_load(in + i0 + k + shift), num, den, direct)) run = mul(run, den);
    }
  });
  Fq inv_run = inv(run);
  for_limbs<K>([&](auto kc) {
    constexpr int k = K - 1 - decltype(kc)::value;
    if (i0 + k < n_out) {
      const G1Affine a = diff_load(in + i0 + k), b = diff_load(in + i0 + k + shift);
      Fq num, den;
      G1Affine r;
      if (diff_slope(a, b, num, den, r)) {
        const Fq lambda = mul(num, mul(inv_run, pre[k]));
        inv_run = mul(inv_run, den);
        r.x = sub(sub(sqr(lambda), a.x), b.x);
        r.y = sub(mul(lambda, sub(b.x, r.x)), b.y);
      }
      diff_store(out + i0 + k, r);
    }
  });
}

__global__ void __launch_bounds__(256) shifted_difference_kernel(G1Affine* __restrict__ out, const G1Affine* __restrict__ in, uint64_t shift, uint64_t n_out) {
  const uint64_t i0 = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) * DIFF_K;
  if (i0 >= n_out) return;
  shifted_difference_lane<DIFF_K>(out, in, i0, shift, n_out);
}

// the ABI's argument rules: the records read are in[0, shift + n_out), the records written out[0, n_out)
bool diff_args_ok(const void* out, const void* in, size_t n_in, size_t shift, size_t n_out, size_t align) {
  if (shift == 0 || shift > n_in || n_out > n_in - shift) return false;
  if (n_out == 0) return true;
  if (!out || !in || ((uintptr_t)out | (uintptr_t)in) % align != 0 || n_in > (~(size_t)0) / sizeof(G1Affine)) return false;
  const uintptr_t o = (uintptr_t)out, i = (uintptr_t)in;
  return o + n_out * sizeof(G1Affine) <= i || i + n_in * sizeof(G1Affine) <= o;
}

}  // namespace

int g1_shifted_difference(void* d_out, const void* d_in, size_t n_in, size_t shift, size_t n_out, hipStream_t st) {
  if (!diff_args_ok(d_out, d_in, n_in, shift, n_out, 16)) return ZK_ERR_BAD_ARGS;   // (16: the kernel's loads)
  if (n_out == 0) return ZK_OK;
  const uint64_t lanes = (n_out + DIFF_K - 1) / DIFF_K, blocks = (lanes + 255) / 256;
  if (blocks >= ((uint64_t)1 << 31)) return ZK_ERR_BAD_ARGS;
  hipLaunchKernelGGL(shifted_difference_kernel, dim3((unsigned)blocks), dim3(256), 0, st, (G1Affine*)d_out, (const G1Affine*)d_in, (uint64_t)shift, (uint64_t)n_out);
  ZK_HIP(hipGetLastError());
  return ZK_OK;
}

int g1_shifted_difference_host(uint64_t* out, const uint64_t* in, size_t n_in, size_t shift, size_t n_out) {
  if (!diff_args_ok(out, in, n_in, shift, n_out, 8)) return ZK_ERR_BAD_ARGS;
  for (uint64_t i0 = 0; i0 < n_out; i0 += DIFF_K)
    shifted_difference_lane<DIFF_K>(reinterpret_cast<G1Affine*>(out), reinterpret_cast<const G1Affine*>(in), i0, shift, n_out);
  return ZK_OK;
}

}  // namespace zk
