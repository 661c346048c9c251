// Fixed-base scalar multiplication over a window table of one base (include/mi355zk.h; the program: fixed_base.hpp): what the reference's
// `Wnaf::base(g, n).scalar(k)` tables are to groth16/generator.rs:178-510, where four G1 vectors, one G2 vector and the H query are all
// multiples of ONE generator.  The table is built once per base by the existing per-point batch_exp (4096 scalars j * 2^(8 w) mod r over the
// same base: no new curve kernel); a multiplication is then one lane per scalar, at most 32 mixed additions from gathered table entries
// into a U-form Jacobian accumulator, X and Y parked in the output record and Z in scratch, and the batched normalisation of batch_exp.
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/mi355zk.h"
#include "fixed_base.hpp"

#include "api_internal.hpp"

namespace zk {
namespace {

// one affine record as whole 16-byte words (the table comes from hipMalloc and its entries are 64 / 128 bytes)
template <class A>
__device__ __forceinline__ A load_record(const A* p) {
  static_assert(sizeof(A) % 16 == 0, "16-byte copies");
  A r;
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint4 v[sizeof(A) / 16];
#pragma unroll
  for (int i = 0; i < (int)(sizeof(A) / 16); ++i) v[i] = q[i];
  __builtin_memcpy(&r, v, sizeof(A));
  return r;
}

// out[i] = (X, Y) of k[i] * P, zbuf[i] = Z (batch_normalize_g1 / _g2 finish the record).  i < n; the scalars of this launch start at
// scalars, the outputs at out: the launcher hands each chunk its own pointers.
template <class G>
__global__ void __launch_bounds__(256) fixed_base_mul_kernel(typename G::Aff* __restrict__ out, const typename G::Aff* __restrict__ table,
                                                            const uint32_t* __restrict__ scalars, uint64_t n, typename G::Z* __restrict__ zbuf,
                                                            int montgomery) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  Fr s;
  {
    const uint4* sp = reinterpret_cast<const uint4*>(scalars + i * 8);
    const uint4 s0 = sp[0], s1 = sp[1];
    s.l[0] = s0.x; s.l[1] = s0.y; s.l[2] = s0.z; s.l[3] = s0.w; s.l[4] = s1.x; s.l[5] = s1.y; s.l[6] = s1.z; s.l[7] = s1.w;
  }
  if (montgomery) s = to_canonical(s);                      // into_repr: one Montgomery product by 1
  const typename G::Acc acc = fixed_base_run<G>(s.l, [&](uint32_t index) { return load_record(table + index); });
  const Jacobian<typename G::Z> r = G::to_std(acc);
  out[i] = typename G::Aff{r.x, r.y};
  zbuf[i] = r.z;
}

// (j << 8 w) mod r, canonical: the value is below 2^255 < 3 r
void table_scalar(int w, int j, uint32_t out[8]) {
  uint32_t v[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  const int bit = FB_WIDTH * w;
  const uint64_t sh = (uint64_t)j << (bit & 31);
  v[bit >> 5] = (uint32_t)sh;
  v[(bit >> 5) + 1] = (uint32_t)(sh >> 32);
  for (int rep = 0; rep < 3; ++rep) {
    bool ge = true;
    for (int l = 7; l >= 0; --l)
      if (v[l] != FrParams::P[l]) {
        ge = v[l] > FrParams::P[l];
        break;
      }
    if (!ge) break;
    uint64_t borrow = 0;
    for (int l = 0; l < 8; ++l) {
      const uint64_t d = (uint64_t)v[l] - FrParams::P[l] - borrow;
      v[l] = (uint32_t)d;
      borrow = (d >> 32) & 1u;
    }
  }
  std::memcpy(out, v, 32);
}

template <class F>
bool base_in_group(const Affine<F>& b) {
  if (b.is_zero()) return false;
  if constexpr (std::is_same<F, Fq>::value) return g1_on_curve_host(b);
  else return g2_in_subgroup_host(b);
}

template <class F>
int table_build(void* d_table, size_t table_bytes, const uint64_t* base_raw, void* stream) {
  if (!d_table || !base_raw || table_bytes < (size_t)FB_ENTRIES * sizeof(Affine<F>)) return ZK_ERR_BAD_ARGS;
  Affine<F> base;
  std::memcpy(&base, base_raw, sizeof base);
  // reducing the table scalars mod r is sound in the order-r group only: E(Fq) is that group, the twist has a cofactor
  if (!base_in_group(base)) return ZK_ERR_BAD_ARGS;
  std::vector<uint32_t> ks((size_t)FB_ENTRIES * 8);
  for (int w = 0; w < FB_WINDOWS; ++w)
    for (int j = 1; j <= FB_HALF; ++j) table_scalar(w, j, &ks[((size_t)w * FB_HALF + (j - 1)) * 8]);
  hipStream_t st = (hipStream_t)stream;
  void* d_in = nullptr;                                     // the base, then the scalars (one-time work: a plain allocation)
  const size_t base_bytes = (sizeof(Affine<F>) + 255) & ~(size_t)255;
  ZK_HIP(hipMalloc(&d_in, base_bytes + ks.size() * 4));
  int rc = ZK_OK;
  if (hipMemcpyAsync(d_in, &base, sizeof base, hipMemcpyHostToDevice, st) != hipSuccess ||
      hipMemcpyAsync((char*)d_in + base_bytes, ks.data(), ks.size() * 4, hipMemcpyHostToDevice, st) != hipSuccess)
    rc = ZK_ERR_DEVICE;
  if (rc == ZK_OK) rc = batch_exp<F>(d_table, d_in, 1, (char*)d_in + base_bytes, 0, (size_t)FB_ENTRIES, stream, nullptr, false, /*g2_trusted=*/true);
  if (hipStreamSynchronize(st) != hipSuccess && rc == ZK_OK) rc = ZK_ERR_DEVICE;
  (void)hipFree(d_in);
  return rc;
}

template <class G>
int table_mul(void* d_out, const void* d_table, const void* d_scalars, size_t n, uint32_t flags, void* stream) {
  using A = typename G::Aff;
  using Z = typename G::Z;
  if (flags & ~MI355ZK_FIXED_SCALARS_MONTGOMERY) return ZK_ERR_BAD_ARGS;
  if (n == 0) return ZK_OK;
  if (!d_out || !d_table || !d_scalars || n >= ((size_t)1 << 31)) return ZK_ERR_BAD_ARGS;
  hipStream_t st = (hipStream_t)stream;
  // chunks of 2^18 lanes, as batch_exp launches them; the Z scratch is one chunk's, reused in stream order
  const size_t chunk = n < ((size_t)1 << 18) ? n : ((size_t)1 << 18);
  std::lock_guard<std::mutex> launch_lk(g_exp_launch_mu);
  void* zbuf = nullptr;
  int rc = exp_scratch((chunk * sizeof(Z) + 255) & ~(size_t)255, stream, &zbuf);
  if (rc) return rc;
  for (size_t i0 = 0; i0 < n; i0 += chunk) {
    const size_t m = n - i0 < chunk ? n - i0 : chunk;
    A* out = (A*)d_out + i0;
    hipLaunchKernelGGL(fixed_base_mul_kernel<G>, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, out, (const A*)d_table,
                       (const uint32_t*)d_scalars + i0 * 8, (uint64_t)m, (Z*)zbuf, (flags & MI355ZK_FIXED_SCALARS_MONTGOMERY) ? 1 : 0);
    ZK_HIP(hipGetLastError());
    rc = std::is_same<G, G1U>::value ? batch_normalize_g1(out, zbuf, m, st) : batch_normalize_g2(out, zbuf, m, st);
    if (rc) return rc;
  }
  return ZK_OK;
}

// ---- the host run of the same program: every entry it needs comes from a plain host scalar multiplication by the table's scalar
// (j << 8 w) mod r (MSB first, leading zeros skipped), kept per base so that a test over many scalars computes an entry once.
template <class F>
Affine<F> host_entry(const Affine<F>& base, uint32_t index) {
  uint32_t k[8];
  table_scalar((int)(index / FB_HALF), (int)(index % FB_HALF) + 1, k);
  const Jacobian<F> b = affine_to_jacobian(base);
  Jacobian<F> res = Jacobian<F>::zero();
  bool found = false;
  for (int i = 255; i >= 0; --i) {
    const bool bit = (k[i >> 5] >> (i & 31)) & 1u;
    if (found) jac_double(res);
    else found = bit;
    if (bit) jac_add(res, b);
  }
  Affine<F> a{F::zero(), F::zero()};
  if (!res.is_zero()) {
    const F zi = inv(res.z), zi2 = sqr(zi);
    a.x = mul(res.x, zi2);
    a.y = mul(res.y, mul(zi2, zi));
  }
  return a;
}

template <class G>
int host_mul(const uint64_t* base_raw, const uint64_t k_raw[4], uint64_t* out_raw) {
  using A = typename G::Aff;
  using F = typename G::Z;
  A base;
  std::memcpy(&base, base_raw, sizeof base);
  if (!base_in_group(base)) return ZK_ERR_BAD_ARGS;
  struct Cache {
    std::vector<A> entry = std::vector<A>(FB_ENTRIES);
    std::vector<uint8_t> have = std::vector<uint8_t>(FB_ENTRIES, 0);
  };
  static std::mutex mu;
  static std::map<std::vector<uint64_t>, Cache> cache;      // by the base's bytes; a handful of bases at most
  std::lock_guard<std::mutex> lk(mu);
  if (cache.size() >= 8) cache.clear();
  Cache& c = cache[std::vector<uint64_t>(base_raw, base_raw + sizeof(A) / 8)];
  uint32_t k[8];
  std::memcpy(k, k_raw, 32);
  const typename G::Acc acc = fixed_base_run<G>(k, [&](uint32_t index) {
    if (!c.have[index]) {
      c.entry[index] = host_entry<F>(base, index);
      c.have[index] = 1;
    }
    return c.entry[index];
  });
  const Jacobian<F> r = G::to_std(acc);
  A a{F::zero(), F::zero()};
  if (!r.is_zero()) {
    const F zi = inv(r.z), zi2 = sqr(zi);
    a.x = mul(r.x, zi2);
    a.y = mul(r.y, mul(zi2, zi));
  }
  std::memcpy(out_raw, &a, sizeof a);
  return ZK_OK;
}

}  // namespace
}  // namespace zk

extern "C" {

size_t mi355zk_fixed_base_table_bytes(int group) {
  return group == 1 ? (size_t)zk::FB_ENTRIES * sizeof(zk::G1Affine) : group == 2 ? (size_t)zk::FB_ENTRIES * sizeof(zk::G2Affine) : 0;
}
int mi355zk_bn254_g1_fixed_base_build_dev(void* d_table, size_t table_bytes, const uint64_t base_affine[8], void* stream) {
  return zk::abi_guard([&]() -> int { return zk::table_build<zk::Fq>(d_table, table_bytes, base_affine, stream); });
}
int mi355zk_bn254_g2_fixed_base_build_dev(void* d_table, size_t table_bytes, const uint64_t base_affine[16], void* stream) {
  return zk::abi_guard([&]() -> int { return zk::table_build<zk::Fq2>(d_table, table_bytes, base_affine, stream); });
}
int mi355zk_bn254_g1_fixed_base_mul_dev(void* d_out_affine, const void* d_table, const void* d_scalars, size_t n, uint32_t flags, void* stream) {
  return zk::abi_guard([&]() -> int { return zk::table_mul<zk::G1U>(d_out_affine, d_table, d_scalars, n, flags, stream); });
}
int mi355zk_bn254_g2_fixed_base_mul_dev(void* d_out_affine, const void* d_table, const void* d_scalars, size_t n, uint32_t flags, void* stream) {
  return zk::abi_guard([&]() -> int { return zk::table_mul<zk::G2U>(d_out_affine, d_table, d_scalars, n, flags, stream); });
}
int mi355zk_selftest_fixed_base_digits(const uint64_t k[4], int16_t digits[32]) {
  return zk::abi_guard([&]() -> int {
    if (!k || !digits) return ZK_ERR_BAD_ARGS;
    uint32_t s[8];
    std::memcpy(s, k, 32);
    uint32_t carry = 0;
    for (int w = 0; w < zk::FB_WINDOWS; ++w) digits[w] = (int16_t)zk::fixed_base_digit(s, w, carry);
    return ZK_OK;
  });
}
int mi355zk_selftest_fixed_base_mul(int group, const uint64_t* base_affine, const uint64_t k[4], uint64_t* out_affine) {
  return zk::abi_guard([&]() -> int {
    if (!base_affine || !k || !out_affine || (group != 1 && group != 2)) return ZK_ERR_BAD_ARGS;
    return group == 1 ? zk::host_mul<zk::G1U>(base_affine, k, out_affine) : zk::host_mul<zk::G2U>(base_affine, k, out_affine);
  });
}

}  // extern "C"
