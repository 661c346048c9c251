// Fixed-base scalar multiplication over a window table of one base (include/mi355zk.h; the program: fixed_base.hpp): what the reference's
// `Wnaf::base(g, n).scalar(k)` tables are to groth16/generator.rs:178-510, where four G1 vectors, one G2 vector and the H query are all
// multiples of ONE generator.  The table is built once per base by the existing per-point batch_exp (4096 scalars j * 2^(8 w) mod r over the
// same base: no new curve kernel); a multiplication is then one lane per scalar, at most 32 mixed additions from gathered table entries
// into a U-form Jacobian accumulator, X and Y parked in the output record and Z in scratch, and the batched normalisation of batch_exp.
// A table SET over several G1 bases (one batch_exp builds all of it) serves linear combinations first + sum_j k[i][j] P_j, one lane per
// (row, slice of bases): the input accumulators of groth16/verifier.rs:44-48 for many proofs against one verifying key.
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <mutex>
#include <type_traits>
#include <vector>

#include "../../include/mi355zk.h"
#include "fixed_base.hpp"

#include "api_internal.hpp"
#include "device_mem.hpp"

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

// ---- out[i] = first + sum_j k[i][j] * P_j over a table SET (table j at entry j * FB_ENTRIES): one lane per (row, slice of slice_len
// consecutive bases), lane t = slice * n + row, so a wave's lanes share their slice and walk the same number of bases.  A lane runs the
// fixed-base program once per base of its slice into ONE accumulator.  n_slices == 1: the lane adds `first` and parks X, Y in out[row], Z
// in zbuf[row] (batch_normalize_g1 finishes the record).  Otherwise the slice's sum goes to partial[t] as a Jacobian record and
// fixed_bases_join_kernel adds a row's slices.  row < n, slice < n_slices; the last slice may be short.
__global__ void __launch_bounds__(256) fixed_bases_lincomb_kernel(G1Affine* __restrict__ out, const G1Affine* __restrict__ tables, uint64_t n_bases,
                                                                 const G1Affine* __restrict__ first, const uint32_t* __restrict__ scalars, uint64_t n,
                                                                 uint64_t slice_len, uint64_t n_slices, Fq* __restrict__ zbuf,
                                                                 G1Jacobian* __restrict__ partial) {
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * n_slices) return;
  const uint64_t slice = t / n, row = t - slice * n;
  const uint64_t j0 = slice * slice_len, j1 = j0 + slice_len < n_bases ? j0 + slice_len : n_bases;
  G1U::Acc acc = G1U::Acc::zero();
#pragma unroll 1
  for (uint64_t j = j0; j < j1; ++j) {
    uint32_t k[8];
    {
      const uint4* sp = reinterpret_cast<const uint4*>(scalars + (row * n_bases + j) * 8);
      const uint4 s0 = sp[0], s1 = sp[1];
      k[0] = s0.x; k[1] = s0.y; k[2] = s0.z; k[3] = s0.w; k[4] = s1.x; k[5] = s1.y; k[6] = s1.z; k[7] = s1.w;
    }
    const G1Affine* table = tables + j * (uint64_t)FB_ENTRIES;
    fixed_base_accumulate<G1U>(acc, k, [&](uint32_t index) { return load_record(table + index); });
  }
  if (n_slices == 1) {
    if (first) fixed_base_add(acc, load_record(first), false);
    const G1Jacobian r = G1U::to_std(acc);
    out[row] = G1Affine{r.x, r.y};
    zbuf[row] = r.z;
  } else {
    partial[t] = G1U::to_std(acc);
  }
}

// out[row] = (X, Y), zbuf[row] = Z of first + sum over the slices of partial[slice * n + row]: the reference's Jacobian addition (jac_add:
// equal, opposite and infinite operands handled), one lane per row
__global__ void __launch_bounds__(256) fixed_bases_join_kernel(G1Affine* __restrict__ out, const G1Affine* __restrict__ first, uint64_t n,
                                                              uint64_t n_slices, Fq* __restrict__ zbuf, const G1Jacobian* __restrict__ partial) {
  const uint64_t row = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  G1Jacobian acc = first ? affine_to_jacobian(load_record(first)) : G1Jacobian::zero();
#pragma unroll 1
  for (uint64_t s = 0; s < n_slices; ++s) jac_add(acc, partial[s * n + row]);
  out[row] = G1Affine{acc.x, acc.y};
  zbuf[row] = acc.z;
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
  // the base, then the scalars (one-time work: a plain allocation).  Declared AFTER `base` and `ks`: on an early error exit its free, which
  DevTemp in;  // waits for the device, runs before those sources of the queued copies die
  const size_t base_bytes = (sizeof(Affine<F>) + 255) & ~(size_t)255;
  if (int rc = in.alloc(base_bytes + ks.size() * 4)) return rc;
  ZK_HIP(hipMemcpyAsync(in.p, &base, sizeof base, hipMemcpyHostToDevice, st));
  ZK_HIP(hipMemcpyAsync(in.as<char>(base_bytes), ks.data(), ks.size() * 4, hipMemcpyHostToDevice, st));
  const int rc = batch_exp<F>(d_table, in.p, 1, in.as<char>(base_bytes), 0, (size_t)FB_ENTRIES, stream, nullptr, false, /*g2_trusted=*/true);
  // the copies out of `base` and `ks` and the build are done with `in`: all three die with this call
  return hipStreamSynchronize(st) != hipSuccess && rc == ZK_OK ? ZK_ERR_DEVICE : rc;
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

// ---- a table SET over n_bases G1 bases, and linear combinations over it
// A row's bases are cut into slices so that one row over a thousand bases does not run on one lane.  Two measured costs set the cut
// (profiles/verify_proofs.md: the A/B): a lane spends about as long on ONE base as the join spends on FB_JOIN_PER_BASE slices, so a
// row's critical path slice_len + n_bases / (FB_JOIN_PER_BASE slice_len) is shortest at slice_len = sqrt(n_bases / FB_JOIN_PER_BASE); and
// past MI355ZK_FIXED_BASES_LANE_TARGET lanes more slices only queue behind one another, so the rows are never cut into more than reach it,
// and not at all when they reach it alone.  Host arithmetic.
constexpr size_t FB_JOIN_PER_BASE = 16;
int bases_plan(size_t n, size_t n_bases, size_t* slice_len, size_t* n_slices) {
  if (!slice_len || !n_slices || n >= ((size_t)1 << 31)) return ZK_ERR_BAD_ARGS;
  if (n_bases == 0) {
    *slice_len = 1;
    *n_slices = 0;
    return ZK_OK;
  }
  const size_t target = MI355ZK_FIXED_BASES_LANE_TARGET, rows = n ? n : 1;
  size_t want = rows >= target ? 1 : (target + rows - 1) / rows;   // rows * want < target + rows < 2^31
  if (want > n_bases) want = n_bases;
  size_t len = (n_bases + want - 1) / want, balance = 1;
  if (n_bases < ((size_t)1 << 31))                                 // (no table set is longer: the loop stays short)
    while (balance * balance * FB_JOIN_PER_BASE < n_bases) ++balance;   // ceil(sqrt(n_bases / FB_JOIN_PER_BASE))
  *slice_len = len > balance ? len : balance;
  *n_slices = (n_bases + *slice_len - 1) / *slice_len;
  return ZK_OK;
}

size_t bases_table_bytes(size_t n_bases) {
  const size_t one = (size_t)FB_ENTRIES * sizeof(G1Affine);
  return n_bases > (((size_t)1 << 31) - 1) / FB_ENTRIES ? 0 : n_bases * one;   // the build's batch_exp indexes its terms with 32 bits
}

int bases_build(void* d_tables, size_t table_bytes, const uint64_t* bases_raw, size_t n_bases, void* stream) {
  if (n_bases == 0) return ZK_OK;
  const size_t need = bases_table_bytes(n_bases);
  if (!d_tables || !bases_raw || need == 0 || table_bytes < need) return ZK_ERR_BAD_ARGS;
  std::vector<G1Affine> bases(n_bases);
  std::memcpy(bases.data(), bases_raw, n_bases * sizeof(G1Affine));
  for (const G1Affine& b : bases)                          // the identity is a base like any other here: its table is all zero
    if (!b.is_zero() && !g1_on_curve_host(b)) return ZK_ERR_BAD_ARGS;
  const size_t total = n_bases * (size_t)FB_ENTRIES;
  std::vector<uint32_t> ks(total * 8), index(total);
  for (int w = 0; w < FB_WINDOWS; ++w)
    for (int j = 1; j <= FB_HALF; ++j) table_scalar(w, j, &ks[((size_t)w * FB_HALF + (j - 1)) * 8]);
  for (size_t b = 0; b < n_bases; ++b) {
    if (b) std::memcpy(&ks[b * FB_ENTRIES * 8], ks.data(), (size_t)FB_ENTRIES * 32);
    for (size_t e = 0; e < (size_t)FB_ENTRIES; ++e) index[b * FB_ENTRIES + e] = (uint32_t)b;
  }
  hipStream_t st = (hipStream_t)stream;
  DevTemp in;  // the bases, the scalars, the base index (one-time work: a plain allocation); declared AFTER the host vectors, as in table_build
  const size_t bases_bytes = (n_bases * sizeof(G1Affine) + 255) & ~(size_t)255, ks_bytes = total * 32;
  if (int rc = in.alloc(bases_bytes + ks_bytes + total * 4)) return rc;
  char* d = in.as<char>();
  ZK_HIP(hipMemcpyAsync(d, bases.data(), n_bases * sizeof(G1Affine), hipMemcpyHostToDevice, st));
  ZK_HIP(hipMemcpyAsync(d + bases_bytes, ks.data(), ks_bytes, hipMemcpyHostToDevice, st));
  ZK_HIP(hipMemcpyAsync(d + bases_bytes + ks_bytes, index.data(), total * 4, hipMemcpyHostToDevice, st));
  const int rc = batch_exp<Fq>(d_tables, d, 0, d + bases_bytes, 0, total, stream, (const uint32_t*)(d + bases_bytes + ks_bytes));
  // the copies out of the host vectors and the build are done with `in`: they all die with this call
  return hipStreamSynchronize(st) != hipSuccess && rc == ZK_OK ? ZK_ERR_DEVICE : rc;
}

int bases_lincomb(void* d_out, const void* d_tables, size_t n_bases, const void* d_first, const void* d_scalars, size_t n, size_t slice_len,
                  void* stream) {
  if (n == 0) return ZK_OK;
  if (!d_out || n >= ((size_t)1 << 31) || (n_bases && (!d_tables || !d_scalars))) return ZK_ERR_BAD_ARGS;
  if (n_bases && (bases_table_bytes(n_bases) == 0 || n > ((size_t)-1) / 32 / n_bases)) return ZK_ERR_BAD_ARGS;
  size_t n_slices = 0;
  if (slice_len == 0) {
    const int rc = bases_plan(n, n_bases, &slice_len, &n_slices);
    if (rc) return rc;
  } else {
    if (slice_len > n_bases) slice_len = n_bases ? n_bases : 1;
    n_slices = (n_bases + slice_len - 1) / slice_len;
  }
  if (n_slices >= ((size_t)1 << 31) || n * n_slices >= ((size_t)1 << 31)) return ZK_ERR_BAD_ARGS;
  hipStream_t st = (hipStream_t)stream;
  // chunks of at most 2^18 lanes, as table_mul launches them (a row's slices stay in one launch); the Z and partial-sum scratch is one
  // chunk's, reused in stream order
  const size_t lanes_max = (size_t)1 << 18, per_row = n_slices > 1 ? n_slices : 1;
  size_t chunk = lanes_max / per_row;
  chunk = chunk < 1 ? 1 : chunk;
  chunk = n < chunk ? n : chunk;
  const size_t z_bytes = (chunk * sizeof(Fq) + 255) & ~(size_t)255;
  const size_t part_bytes = n_slices > 1 ? chunk * n_slices * sizeof(G1Jacobian) : 0;
  std::lock_guard<std::mutex> launch_lk(g_exp_launch_mu);
  void* scratch = nullptr;
  int rc = exp_scratch(z_bytes + part_bytes, stream, &scratch);
  if (rc) return rc;
  Fq* zbuf = (Fq*)scratch;
  G1Jacobian* partial = (G1Jacobian*)((char*)scratch + z_bytes);
  for (size_t i0 = 0; i0 < n; i0 += chunk) {
    const size_t m = n - i0 < chunk ? n - i0 : chunk;
    G1Affine* out = (G1Affine*)d_out + i0;
    const size_t lanes = m * n_slices;
    if (lanes)
      hipLaunchKernelGGL(fixed_bases_lincomb_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, out, (const G1Affine*)d_tables,
                         (uint64_t)n_bases, (const G1Affine*)d_first, (const uint32_t*)d_scalars + i0 * n_bases * 8, (uint64_t)m,
                         (uint64_t)slice_len, (uint64_t)n_slices, zbuf, partial);
    if (n_slices != 1)
      hipLaunchKernelGGL(fixed_bases_join_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, st, out, (const G1Affine*)d_first, (uint64_t)m,
                         (uint64_t)n_slices, zbuf, (const G1Jacobian*)partial);
    ZK_HIP(hipGetLastError());
    rc = batch_normalize_g1(out, zbuf, m, st);
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

// the entries of one base, computed on demand and kept by the base's bytes (a handful of bases at most).  The caller holds g_host_mu.
template <class A>
struct HostCache {
  std::vector<A> entry = std::vector<A>(FB_ENTRIES);
  std::vector<uint8_t> have = std::vector<uint8_t>(FB_ENTRIES, 0);
};
std::mutex g_host_mu;
template <class G>
HostCache<typename G::Aff>& host_cache(const uint64_t* base_raw) {
  using A = typename G::Aff;
  static std::map<std::vector<uint64_t>, HostCache<A>> cache;
  const std::vector<uint64_t> key(base_raw, base_raw + sizeof(A) / 8);
  auto it = cache.find(key);
  if (it != cache.end()) return it->second;
  if (cache.size() >= 8) cache.clear();
  return cache[key];
}
template <class G>
void host_accumulate(typename G::Acc& acc, const typename G::Aff& base, HostCache<typename G::Aff>& c, const uint64_t k_raw[4]) {
  uint32_t k[8];
  std::memcpy(k, k_raw, 32);
  fixed_base_accumulate<G>(acc, k, [&](uint32_t index) {
    if (!c.have[index]) {
      c.entry[index] = host_entry<typename G::Z>(base, index);
      c.have[index] = 1;
    }
    return c.entry[index];
  });
}
template <class G>
void host_finish(const typename G::Acc& acc, uint64_t* out_raw) {
  using A = typename G::Aff;
  using F = typename G::Z;
  const Jacobian<F> r = G::to_std(acc);
  A a{F::zero(), F::zero()};
  if (!r.is_zero()) {
    const F zi = inv(r.z), zi2 = sqr(zi);
    a.x = mul(r.x, zi2);
    a.y = mul(r.y, mul(zi2, zi));
  }
  std::memcpy(out_raw, &a, sizeof a);
}

template <class G>
int host_mul(const uint64_t* base_raw, const uint64_t k_raw[4], uint64_t* out_raw) {
  typename G::Aff base;
  std::memcpy(&base, base_raw, sizeof base);
  if (!base_in_group(base)) return ZK_ERR_BAD_ARGS;
  std::lock_guard<std::mutex> lk(g_host_mu);
  typename G::Acc acc = G::Acc::zero();
  host_accumulate<G>(acc, base, host_cache<G>(base_raw), k_raw);
  host_finish<G>(acc, out_raw);
  return ZK_OK;
}

// one row of bases_lincomb on the host: the program of the one-slice lane (every base into one accumulator, then `first`)
int host_lincomb(const uint64_t* bases_raw, size_t n_bases, const uint64_t* first_raw, const uint64_t* scalars, uint64_t out_raw[8]) {
  if (!out_raw || (n_bases && (!bases_raw || !scalars))) return ZK_ERR_BAD_ARGS;
  std::vector<G1Affine> bases(n_bases);
  if (n_bases) std::memcpy(bases.data(), bases_raw, n_bases * sizeof(G1Affine));
  for (const G1Affine& b : bases)
    if (!b.is_zero() && !g1_on_curve_host(b)) return ZK_ERR_BAD_ARGS;
  std::lock_guard<std::mutex> lk(g_host_mu);
  G1U::Acc acc = G1U::Acc::zero();
  for (size_t j = 0; j < n_bases; ++j)
    if (!bases[j].is_zero())                                // (the identity's table is all zero: every entry is skipped)
      host_accumulate<G1U>(acc, bases[j], host_cache<G1U>(bases_raw + 8 * j), scalars + 4 * j);
  if (first_raw) {
    G1Affine first;
    std::memcpy(&first, first_raw, sizeof first);
    fixed_base_add(acc, first, false);
  }
  host_finish<G1U>(acc, out_raw);
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
size_t mi355zk_fixed_bases_table_bytes(size_t n_bases) { return zk::bases_table_bytes(n_bases); }
int mi355zk_fixed_bases_plan(size_t n, size_t n_bases, size_t* slice_len, size_t* n_slices) {
  return zk::abi_guard([&]() -> int { return zk::bases_plan(n, n_bases, slice_len, n_slices); });
}
int mi355zk_bn254_g1_fixed_bases_build_dev(void* d_tables, size_t table_bytes, const uint64_t* bases_affine, size_t n_bases, void* stream) {
  return zk::abi_guard([&]() -> int { return zk::bases_build(d_tables, table_bytes, bases_affine, n_bases, stream); });
}
int mi355zk_bn254_g1_fixed_bases_lincomb_dev(void* d_out_affine, const void* d_tables, size_t n_bases, const void* d_first_affine,
                                             const void* d_scalars, size_t n, size_t slice_len, void* stream) {
  return zk::abi_guard([&]() -> int { return zk::bases_lincomb(d_out_affine, d_tables, n_bases, d_first_affine, d_scalars, n, slice_len, stream); });
}
int mi355zk_selftest_fixed_bases_lincomb(const uint64_t* bases_affine, size_t n_bases, const uint64_t* first_affine, const uint64_t* scalars,
                                         uint64_t out_affine[8]) {
  return zk::abi_guard([&]() -> int { return zk::host_lincomb(bases_affine, n_bases, first_affine, scalars, out_affine); });
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
