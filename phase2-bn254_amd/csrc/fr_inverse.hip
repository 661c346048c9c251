// Fr batch inversion on the device: out[i] = in[i]^-1 for a device-resident vector, Montgomery's trick over the run / tile shape of
// fr_poly.hip (fr_inverse.hpp: the lane routines and the product tree).  Three launches and ONE Fermat inversion per call, the launches
// being the only synchronisation between workgroups -- no flags, no look-back, no cooperative launch:
//   1  fr_inverse_products_kernel  every lane's run product, the product tree of the tile going up, one product per tile; the zeros counted
//   2  fr_inverse_carry_kernel     ONE workgroup walks the tile products INV_CARRY_W at a time: going up it keeps the product of all the chunks
//                                  before each chunk, lane 0 inverts the total (the call's only inv(), ~380 dependent products), coming back
//                                  down every chunk's tree turns (chunks 0 .. c)^-1 and the product before it into the inverse of every tile
//   3  fr_inverse_apply_kernel     every tile redoes its run prefixes and its tree, seeds the root with its tile inverse, walks the tree down
//                                  to the inverse of every run product and back-substitutes
// Variant (b), MI355ZK_INV_ONE_LAUNCH: launch 3 alone, lane 0 of every tile inverting the tile's own product between the two halves of the
// tree.  Both were measured (profiles/kzg_evals.md); the library ships the three launches.
// blockIdx.y is a ROW: fr_evals.hip inverts the B rows of its denominators with one call, and still one inversion.  Every product returns the
// canonical residue, so the results are the unique inverses byte for byte whatever the grouping.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/mi355zk.h"
#include "api_internal.hpp"
#include "device_mem.hpp"
#include "fr_inverse.hpp"

namespace zk {
namespace {

constexpr int INV_WAVE = 64;

// The tree going up: s[W + lane] = mine, then every level's nodes from their children.  On return s[1] is the product of all the lanes'
// values and all lanes have passed a barrier.
template <int LOG_W>
__device__ __forceinline__ void inv_tree_up(Fr* s, const Fr& mine) {
  constexpr int W = 1 << LOG_W;
  const int tid = threadIdx.x;
  s[W + tid] = mine;
  __syncthreads();
#pragma unroll 1
  for (int lvl = LOG_W - 1; lvl >= 0; --lvl) {
    const int m = 1 << lvl;
    if (tid < m) s[m + tid] = mul(s[2 * (m + tid)], s[2 * (m + tid) + 1]);
    __syncthreads();
  }
}
// The tree coming down: s[1] holds the inverse of the root's product (written before a barrier).  Every child becomes its parent's inverse
// times its sibling's product; both children read before either is written.  Returns the inverse of the lane's own leaf; the leaves
// themselves are not written back.
template <int LOG_W>
__device__ __forceinline__ Fr inv_tree_down(Fr* s) {
  constexpr int W = 1 << LOG_W;
  const int tid = threadIdx.x;
#pragma unroll 1
  for (int lvl = 0; lvl < LOG_W - 1; ++lvl) {
    const int cnt = 2 << lvl;   // the children of level lvl: nodes cnt .. 2 cnt - 1
    Fr val;
    if (tid < cnt) val = mul(s[(cnt + tid) >> 1], s[(cnt + tid) ^ 1]);
    __syncthreads();
    if (tid < cnt) s[cnt + tid] = val;
    __syncthreads();
  }
  return mul(s[(W + tid) >> 1], s[(W + tid) ^ 1]);
}

// as fr_r1cs_check_kernel counts failures: one ballot per wave, and only a wave that saw a zero sums its lanes' counts and adds them
__device__ __forceinline__ void inv_count_zeros(uint32_t zeros, uint32_t* n_zero) {
  const unsigned long long mask = __ballot(zeros != 0);
  if (mask != 0) {
    uint32_t c = (uint32_t)__builtin_popcount(zeros);
#pragma unroll
    for (int off = INV_WAVE / 2; off >= 1; off >>= 1) c += __shfl_xor(c, off, INV_WAVE);
    if (threadIdx.x % INV_WAVE == 0) atomicAdd(n_zero, c);
  }
}

__global__ void __launch_bounds__(INV_WG) fr_inverse_products_kernel(Fr* __restrict__ tprod, const Fr* __restrict__ in, uint64_t n, uint64_t stride,
                                                                     uint32_t n_tiles, uint32_t* n_zero) {
  __shared__ __align__(16) Fr s[2 * INV_WG];
  const uint64_t lo = ((uint64_t)blockIdx.x * INV_WG + threadIdx.x) * INV_RUN;
  Fr v[INV_RUN];
  const uint32_t zeros = inv_run_load(v, in + (uint64_t)blockIdx.y * stride, lo, n);
  if (n_zero != nullptr) inv_count_zeros(zeros, n_zero);
  inv_tree_up<INV_LOG_WG>(s, inv_run_product(v));
  if (threadIdx.x == 0) poly_st(tprod + (uint64_t)blockIdx.y * n_tiles + blockIdx.x, s[1]);
}

// tprod: n_tiles tile products in, their inverses out.  before: one element per chunk (the product of the chunks before it).
__global__ void __launch_bounds__(INV_CARRY_W) fr_inverse_carry_kernel(Fr* __restrict__ tprod, Fr* __restrict__ before, uint32_t n_tiles) {
  __shared__ __align__(16) Fr s[2 * INV_CARRY_W];   // (node 0 of the heap is free: the broadcast slot)
  const int tid = threadIdx.x;
  const uint32_t n_chunks = (n_tiles + INV_CARRY_W - 1) / INV_CARRY_W;
  Fr carry = Fr::one();   // every lane keeps the same running product
#pragma unroll 1
  for (uint32_t c = 0; c < n_chunks; ++c) {
    const uint64_t tile = (uint64_t)c * INV_CARRY_W + tid;
    inv_tree_up<INV_LOG_CARRY>(s, tile < n_tiles ? poly_ld(tprod + tile) : Fr::one());
    if (tid == 0) poly_st(before + c, carry);
    carry = mul(carry, s[1]);
    if (c + 1 != n_chunks) __syncthreads();   // s[1] is read before the next chunk's tree writes it; the last tree stays for the way down
  }
  if (tid == 0) s[0] = inv(carry);
  __syncthreads();   // (also orders lane 0's stores to `before` ahead of the loads below)
  Fr J = s[0];
#pragma unroll 1
  for (int64_t c = (int64_t)n_chunks - 1; c >= 0; --c) {
    const uint64_t tile = (uint64_t)c * INV_CARRY_W + tid;
    if ((uint32_t)c + 1 != n_chunks) inv_tree_up<INV_LOG_CARRY>(s, tile < n_tiles ? poly_ld(tprod + tile) : Fr::one());
    const Fr chunk = s[1];
    __syncthreads();
    if (tid == 0) s[1] = mul(J, poly_ld(before + c));
    __syncthreads();
    const Fr mine = inv_tree_down<INV_LOG_CARRY>(s);
    if (tile < n_tiles) poly_st(tprod + tile, mine);
    J = mul(J, chunk);
    __syncthreads();   // the tree is read before the next chunk's leaves are written
  }
}

// OWN_INV: variant (b) -- tinv is not read, lane 0 inverts the tile's product
template <bool OWN_INV>
__global__ void __launch_bounds__(INV_WG) fr_inverse_apply_kernel(Fr* out, const Fr* in, const Fr* __restrict__ tinv, uint64_t n, uint64_t stride,
                                                                  uint32_t n_tiles, uint32_t* n_zero) {
  __shared__ __align__(16) Fr s[2 * INV_WG];
  const uint64_t lo = ((uint64_t)blockIdx.x * INV_WG + threadIdx.x) * INV_RUN;
  const uint64_t row = (uint64_t)blockIdx.y * stride;
  Fr v[INV_RUN], pre[INV_RUN];
  const uint32_t zeros = inv_run_load(v, in + row, lo, n);
  if (OWN_INV && n_zero != nullptr) inv_count_zeros(zeros, n_zero);
  inv_run_prefix(pre, v);
  inv_tree_up<INV_LOG_WG>(s, pre[INV_RUN - 1]);
  if (threadIdx.x == 0) s[1] = OWN_INV ? inv(s[1]) : poly_ld(tinv + (uint64_t)blockIdx.y * n_tiles + blockIdx.x);
  __syncthreads();
  const Fr J = inv_tree_down<INV_LOG_WG>(s);
  inv_run_apply(out + row, v, pre, zeros, lo, n, J);   // (out may be in: a lane stores only what it loaded)
}

// the tile products / inverses and the chunk prefixes of one call: per (device, stream), under g_inv_mu from get() until the call's last
// launch is enqueued (device_mem.hpp: StreamScratch)
std::mutex g_inv_mu;
StreamScratch g_inv_scratch;

// n >= 1, rows >= 1; the arguments have been checked
int inverse_run(Fr* d_out, const Fr* d_in, size_t n, size_t stride, size_t rows, uint32_t* d_n_zero, hipStream_t st) {
  const uint32_t n_tiles = (uint32_t)((n + INV_TILE - 1) / INV_TILE);
  const uint64_t all_tiles = (uint64_t)n_tiles * rows;
  if (all_tiles >= (1ull << 32)) return ZK_ERR_BAD_ARGS;
  const dim3 grid(n_tiles, (unsigned)rows);
  if (INV_ONE_LAUNCH) {
    hipLaunchKernelGGL(fr_inverse_apply_kernel<true>, grid, dim3(INV_WG), 0, st, d_out, d_in, (const Fr*)nullptr, (uint64_t)n, (uint64_t)stride, n_tiles,
                       d_n_zero);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
  }
  const uint64_t n_chunks = (all_tiles + INV_CARRY_W - 1) / INV_CARRY_W;
  int dev = 0;
  ZK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_inv_mu);
  void* p = nullptr;
  if (int rc = g_inv_scratch.get(dev, st, (all_tiles + n_chunks) * sizeof(Fr), &p)) return rc;
  Fr* tprod = (Fr*)p;
  Fr* before = tprod + all_tiles;
  hipLaunchKernelGGL(fr_inverse_products_kernel, grid, dim3(INV_WG), 0, st, tprod, d_in, (uint64_t)n, (uint64_t)stride, n_tiles, d_n_zero);
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(fr_inverse_carry_kernel, dim3(1), dim3(INV_CARRY_W), 0, st, tprod, before, (uint32_t)all_tiles);
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(fr_inverse_apply_kernel<false>, grid, dim3(INV_WG), 0, st, d_out, d_in, (const Fr*)tprod, (uint64_t)n, (uint64_t)stride, n_tiles,
                     (uint32_t*)nullptr);
  ZK_HIP(hipGetLastError());
  return ZK_OK;
}

}  // namespace

int fr_inverse_rows(Fr* d_io, size_t n, size_t stride, size_t rows, hipStream_t st, uint32_t* d_n_zero) {
  if (n == 0 || rows == 0) return ZK_OK;
  if ((uint64_t)n >= (1ull << 32) || rows > 65535 || stride < n) return ZK_ERR_BAD_ARGS;
  return inverse_run(d_io, d_io, n, stride, rows, d_n_zero, st);
}

void fr_inverse_release_all() {
  std::lock_guard<std::mutex> lk(g_inv_mu);
  g_inv_scratch.release_all();
}

}  // namespace zk

extern "C" {

int mi355zk_bn254_fr_batch_inverse_dev(void* d_out, const void* d_in, size_t n, uint32_t* d_n_zero, void* stream) {
  return zk::abi_guard([&]() -> int {
    if ((uint64_t)n >= (1ull << 32) || (n && (!d_out || !d_in))) return ZK_ERR_BAD_ARGS;
    if (n && d_out != d_in) {
      const uintptr_t o = (uintptr_t)d_out, i = (uintptr_t)d_in, bytes = (uintptr_t)n * 32;
      if (o + bytes < o || i + bytes < i || (o < i + bytes && i < o + bytes)) return ZK_ERR_BAD_ARGS;
    }
    if (d_n_zero) ZK_HIP(hipMemsetAsync(d_n_zero, 0, sizeof(uint32_t), (hipStream_t)stream));
    if (n == 0) return ZK_OK;
    return zk::inverse_run((zk::Fr*)d_out, (const zk::Fr*)d_in, n, n, 1, d_n_zero, (hipStream_t)stream);
  });
}

int mi355zk_selftest_fr_batch_inverse(uint64_t* out, const uint64_t* in, size_t n, uint32_t* n_zero) {
  return zk::abi_guard([&]() -> int {
    if ((uint64_t)n >= (1ull << 32) || (n && (!out || !in))) return ZK_ERR_BAD_ARGS;
    const uint32_t zeros = n ? zk::inv_batch_host((zk::Fr*)out, (const zk::Fr*)in, n) : 0;
    if (n_zero) *n_zero = zeros;
    return ZK_OK;
  });
}

int mi355zk_fr_inverse_geometry(uint32_t* run, uint32_t* tile, uint32_t* carry_width) {
  return zk::abi_guard([&]() -> int {
    if (!run || !tile || !carry_width) return ZK_ERR_BAD_ARGS;
    *run = zk::INV_RUN;
    *tile = zk::INV_TILE;
    *carry_width = zk::INV_CARRY_W;
    return ZK_OK;
  });
}

}  // extern "C"
