// Fr polynomials against one point: division by (x - z) and evaluation at z on device-resident coefficients, for many points per call.
//   kate_divison                     bellman/src/sonic/util.rs:444-463   (a serial recurrence there)
//   evaluate_at_consequitive_powers  bellman/src/sonic/util.rs:151-200   (first_power = 1)
// The recurrence H[i] = a[i] + z H[i+1] is a suffix scan (fr_poly.hpp); it runs as reduce-then-scan in THREE launches, and the launches are
// the only synchronisation between workgroups -- no flags, no look-back, no cooperative launch:
//   1  fr_poly_aggregate_kernel  every lane's run value, a log-step suffix scan over the lanes in LDS, one aggregate per tile
//   2  fr_poly_carry_kernel      one workgroup per point scans the tile aggregates from the top tile down, POLY_CARRY_W tiles at a time with a
//                                running carry: agg[t] becomes H[t * POLY_TILE], and H[0] = a(z) is the remainder
//   3  fr_poly_apply_kernel      every tile repeats launch 1 with the tile above's H seeded into its top lane, which makes the scan's values the
//                                H at the bottom of every run; then every lane re-runs its chain from the H above it and stores q
// Evaluation is launches 1 and 2.  blockIdx.y is the point; every point has its table of squarings (fr_poly_points_kernel builds them on the
// device from the points, which travel by value in the launch arguments, 64 per launch).  Every field step returns the canonical residue, so
// q and the remainder are the reference's byte for byte however the sums are associated.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <vector>

#include "../../include/mi355zk.h"
#include "api_internal.hpp"
#include "device_mem.hpp"
#include "fr_poly.hpp"

namespace zk {
namespace {

static_assert(MI355ZK_POLY_MAX_POINTS == 65535, "blockIdx.y is the point index");
constexpr int POLY_POINTS_PER_LAUNCH = 64;   // 2 KB of launch arguments
struct FrPolyZs {
  Fr z[POLY_POINTS_PER_LAUNCH];
};

__global__ void __launch_bounds__(POLY_POINTS_PER_LAUNCH) fr_poly_points_kernel(FrPolyPoint* __restrict__ tab, const FrPolyZs zs, uint32_t m) {
  if (threadIdx.x >= m) return;
  Fr cur = zs.z[threadIdx.x];
  Fr* out = tab[threadIdx.x].sq;
#pragma unroll 1
  for (int j = 0; j < POLY_SQ; ++j) {
    poly_st(out + j, cur);
    cur = sqr(cur);
  }
}

// Suffix scan over the 2^log_w lanes of the workgroup: returns mine + sum_{d >= 1} m^d (lane + d's value), m = sq[0], with sq[k] = m^(2^k).
// On return s[lane] holds every lane's result and all lanes have passed a barrier.
__device__ __forceinline__ Fr poly_lane_scan(Fr* s, Fr mine, const Fr* __restrict__ sq, int log_w) {
  const int tid = threadIdx.x, w = 1 << log_w;
  s[tid] = mine;
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < log_w; ++k) {
    const int d = 1 << k;
    const bool has = tid + d < w;
    const Fr up = s[has ? tid + d : tid];
    __syncthreads();
    if (has) {
      mine = poly_combine(mine, sq[k], up);
      s[tid] = mine;
    }
    __syncthreads();
  }
  return mine;
}

__global__ void __launch_bounds__(POLY_WG) fr_poly_aggregate_kernel(Fr* __restrict__ agg, const FrPolyPoint* __restrict__ tab, const Fr* __restrict__ a,
                                                                    uint64_t n, uint32_t n_tiles) {
  __shared__ __align__(16) Fr s[POLY_WG];
  const FrPolyPoint* t = tab + blockIdx.y;
  const uint64_t lo = ((uint64_t)blockIdx.x * POLY_WG + threadIdx.x) * POLY_RUN;
  Fr v[POLY_RUN];
  poly_run_load(v, a, lo, n);
  const Fr mine = poly_lane_scan(s, poly_run_value(v, t->sq[0], Fr::zero()), t->sq + POLY_LOG_RUN, POLY_LOG_WG);
  if (threadIdx.x == 0) poly_st(agg + (uint64_t)blockIdx.y * n_tiles + blockIdx.x, mine);
}

__global__ void __launch_bounds__(POLY_CARRY_W) fr_poly_carry_kernel(Fr* __restrict__ agg, Fr* __restrict__ rem, const FrPolyPoint* __restrict__ tab,
                                                                     uint32_t n_tiles) {
  __shared__ __align__(16) Fr s[POLY_CARRY_W];
  const FrPolyPoint* t = tab + blockIdx.y;
  Fr* A = agg + (uint64_t)blockIdx.y * n_tiles;
  Fr carry = Fr::zero();   // H at the bottom of the chunk above
#pragma unroll 1
  for (int64_t c = ((int64_t)n_tiles - 1) / POLY_CARRY_W; c >= 0; --c) {
    const uint64_t tile = (uint64_t)c * POLY_CARRY_W + threadIdx.x;
    Fr mine = tile < n_tiles ? poly_ld(A + tile) : Fr::zero();
    if (threadIdx.x == POLY_CARRY_W - 1) mine = poly_combine(mine, t->sq[POLY_LOG_TILE], carry);
    mine = poly_lane_scan(s, mine, t->sq + POLY_LOG_TILE, POLY_LOG_CARRY);
    if (tile < n_tiles) poly_st(A + tile, mine);
    carry = s[0];
    __syncthreads();   // s[0] is read before the next chunk's scan writes it
  }
  if (threadIdx.x == 0 && rem != nullptr) poly_st(rem + blockIdx.y, carry);
}

__global__ void __launch_bounds__(POLY_WG) fr_poly_apply_kernel(Fr* __restrict__ q, uint64_t q_stride, const Fr* __restrict__ agg,
                                                                const FrPolyPoint* __restrict__ tab, const Fr* __restrict__ a, uint64_t n, uint32_t n_tiles) {
  __shared__ __align__(16) Fr s[POLY_WG];
  const FrPolyPoint* t = tab + blockIdx.y;
  const uint64_t lo = ((uint64_t)blockIdx.x * POLY_WG + threadIdx.x) * POLY_RUN;
  const bool top = threadIdx.x == POLY_WG - 1;
  Fr v[POLY_RUN];
  poly_run_load(v, a, lo, n);
  // H at the bottom of the tile above (launch 2); only the top lane's chain starts from it
  const Fr above = blockIdx.x + 1 < n_tiles ? poly_ld(agg + (uint64_t)blockIdx.y * n_tiles + blockIdx.x + 1) : Fr::zero();
  const Fr z = t->sq[0];
  poly_lane_scan(s, poly_run_value(v, z, top ? above : Fr::zero()), t->sq + POLY_LOG_RUN, POLY_LOG_WG);
  const Fr seed = top ? above : s[threadIdx.x + 1];
  poly_run_apply(q + (uint64_t)blockIdx.y * q_stride, v, lo, n, z, seed);
}

// the tables of squarings and the tile aggregates of one call: per (device, stream), under g_poly_mu from get() until the call's last launch
// is enqueued (device_mem.hpp: StreamScratch)
std::mutex g_poly_mu;
StreamScratch g_poly_scratch;

// d_q == nullptr: evaluation only.  n >= 1; the arguments have been checked.
int poly_run(Fr* d_q, size_t q_stride, Fr* d_rem, const Fr* d_a, size_t n, const uint64_t* z, size_t n_points, hipStream_t st) {
  const uint32_t n_tiles = (uint32_t)((n + POLY_TILE - 1) / POLY_TILE);
  const size_t tab_bytes = (n_points * sizeof(FrPolyPoint) + 255) & ~(size_t)255;
  const size_t agg_bytes = n_points * (size_t)n_tiles * sizeof(Fr);
  int dev = 0;
  ZK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_poly_mu);
  void* p = nullptr;
  if (int rc = g_poly_scratch.get(dev, st, tab_bytes + agg_bytes, &p)) return rc;
  FrPolyPoint* tab = (FrPolyPoint*)p;
  Fr* agg = (Fr*)((char*)p + tab_bytes);
  FrPolyZs zs;
  for (size_t p0 = 0; p0 < n_points; p0 += POLY_POINTS_PER_LAUNCH) {
    const size_t m = n_points - p0 < (size_t)POLY_POINTS_PER_LAUNCH ? n_points - p0 : (size_t)POLY_POINTS_PER_LAUNCH;
    std::memcpy(zs.z, z + p0 * 4, m * 32);
    hipLaunchKernelGGL(fr_poly_points_kernel, dim3(1), dim3(POLY_POINTS_PER_LAUNCH), 0, st, tab + p0, zs, (uint32_t)m);
  }
  ZK_HIP(hipGetLastError());
  const dim3 grid(n_tiles, (unsigned)n_points);
  hipLaunchKernelGGL(fr_poly_aggregate_kernel, grid, dim3(POLY_WG), 0, st, agg, tab, d_a, (uint64_t)n, n_tiles);
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(fr_poly_carry_kernel, dim3(1, (unsigned)n_points), dim3(POLY_CARRY_W), 0, st, agg, d_rem, tab, n_tiles);
  ZK_HIP(hipGetLastError());
  if (d_q != nullptr && n >= 2) {
    hipLaunchKernelGGL(fr_poly_apply_kernel, grid, dim3(POLY_WG), 0, st, d_q, (uint64_t)q_stride, agg, tab, d_a, (uint64_t)n, n_tiles);
    ZK_HIP(hipGetLastError());
  }
  return ZK_OK;
}

// The three launches on the host, one point: the same lanes, tiles and chunks, every combine step in the kernels' order.
void poly_scan_host(Fr* s, int log_w, const Fr* sq) {
  const int w = 1 << log_w;
  std::vector<Fr> old(w);
  for (int k = 0; k < log_w; ++k) {
    const int d = 1 << k;
    std::memcpy(old.data(), s, sizeof(Fr) * w);
    for (int l = 0; l + d < w; ++l) s[l] = poly_combine(old[l], sq[k], old[l + d]);
  }
}
void poly_divide_host(Fr* q, Fr* rem, const Fr* a, size_t n, const Fr& z) {
  FrPolyPoint t;
  poly_point_fill(t, z);
  const size_t n_tiles = (n + POLY_TILE - 1) / POLY_TILE;
  std::vector<Fr> agg(n_tiles), s(POLY_WG > POLY_CARRY_W ? POLY_WG : POLY_CARRY_W);
  Fr v[POLY_RUN];
  for (size_t tile = 0; tile < n_tiles; ++tile) {   // launch 1
    for (int l = 0; l < POLY_WG; ++l) {
      poly_run_load(v, a, (tile * POLY_WG + l) * POLY_RUN, n);
      s[l] = poly_run_value(v, t.sq[0], Fr::zero());
    }
    poly_scan_host(s.data(), POLY_LOG_WG, t.sq + POLY_LOG_RUN);
    agg[tile] = s[0];
  }
  Fr carry = Fr::zero();
  for (int64_t c = ((int64_t)n_tiles - 1) / POLY_CARRY_W; c >= 0; --c) {   // launch 2
    for (int l = 0; l < POLY_CARRY_W; ++l) {
      const size_t tile = (size_t)c * POLY_CARRY_W + l;
      s[l] = tile < n_tiles ? agg[tile] : Fr::zero();
    }
    s[POLY_CARRY_W - 1] = poly_combine(s[POLY_CARRY_W - 1], t.sq[POLY_LOG_TILE], carry);
    poly_scan_host(s.data(), POLY_LOG_CARRY, t.sq + POLY_LOG_TILE);
    for (int l = 0; l < POLY_CARRY_W; ++l)
      if ((size_t)c * POLY_CARRY_W + l < n_tiles) agg[(size_t)c * POLY_CARRY_W + l] = s[l];
    carry = s[0];
  }
  *rem = carry;
  if (n < 2) return;
  for (size_t tile = 0; tile < n_tiles; ++tile) {   // launch 3
    const Fr above = tile + 1 < n_tiles ? agg[tile + 1] : Fr::zero();
    for (int l = 0; l < POLY_WG; ++l) {
      poly_run_load(v, a, (tile * POLY_WG + l) * POLY_RUN, n);
      s[l] = poly_run_value(v, t.sq[0], l == POLY_WG - 1 ? above : Fr::zero());
    }
    poly_scan_host(s.data(), POLY_LOG_WG, t.sq + POLY_LOG_RUN);
    for (int l = 0; l < POLY_WG; ++l) {
      const uint64_t lo = (tile * POLY_WG + l) * POLY_RUN;
      poly_run_load(v, a, lo, n);
      poly_run_apply(q, v, lo, n, t.sq[0], l == POLY_WG - 1 ? above : s[l + 1]);
    }
  }
}

// what both device entry points refuse (include/mi355zk.h: rc 3), their own output pointers apart
bool poly_args_ok(const void* d_coeffs, size_t n, const uint64_t* z, size_t n_points) {
  if ((uint64_t)n >= (1ull << 32) || n_points == 0 || n_points > MI355ZK_POLY_MAX_POINTS) return false;
  return z != nullptr && (n == 0 || d_coeffs != nullptr);
}

}  // namespace

void fr_poly_release_all() {
  std::lock_guard<std::mutex> lk(g_poly_mu);
  g_poly_scratch.release_all();
}

}  // namespace zk

extern "C" {

int mi355zk_bn254_fr_poly_eval_dev(void* d_out, const void* d_coeffs, size_t n, const uint64_t* z, size_t n_points, void* stream) {
  return zk::abi_guard([&]() -> int {
    if (!zk::poly_args_ok(d_coeffs, n, z, n_points) || !d_out) return ZK_ERR_BAD_ARGS;
    if (n == 0) {
      ZK_HIP(hipMemsetAsync(d_out, 0, n_points * 32, (hipStream_t)stream));
      return ZK_OK;
    }
    return zk::poly_run(nullptr, 0, (zk::Fr*)d_out, (const zk::Fr*)d_coeffs, n, z, n_points, (hipStream_t)stream);
  });
}

int mi355zk_bn254_fr_poly_divide_dev(void* d_q, size_t q_stride, void* d_rem, const void* d_coeffs, size_t n, const uint64_t* z, size_t n_points,
                                     void* stream) {
  return zk::abi_guard([&]() -> int {
    if (!zk::poly_args_ok(d_coeffs, n, z, n_points)) return ZK_ERR_BAD_ARGS;
    const size_t qn = n ? n - 1 : 0;
    if (q_stride < qn || (qn && !d_q)) return ZK_ERR_BAD_ARGS;
    if (qn) {
      if (q_stride > ((size_t)-1 / 64) / n_points) return ZK_ERR_BAD_ARGS;   // the quotient range would wrap the address space
      const uintptr_t q_lo = (uintptr_t)d_q, q_hi = q_lo + ((n_points - 1) * q_stride + qn) * 32;
      const uintptr_t a_lo = (uintptr_t)d_coeffs, a_hi = a_lo + n * 32;
      if (q_hi < q_lo || (q_lo < a_hi && a_lo < q_hi)) return ZK_ERR_BAD_ARGS;
    }
    if (n == 0) {
      if (d_rem) ZK_HIP(hipMemsetAsync(d_rem, 0, n_points * 32, (hipStream_t)stream));
      return ZK_OK;
    }
    return zk::poly_run((zk::Fr*)d_q, q_stride, (zk::Fr*)d_rem, (const zk::Fr*)d_coeffs, n, z, n_points, (hipStream_t)stream);
  });
}

int mi355zk_selftest_fr_poly_divide(uint64_t* q, uint64_t rem[4], const uint64_t* coeffs, size_t n, const uint64_t z[4]) {
  return zk::abi_guard([&]() -> int {
    if ((uint64_t)n >= (1ull << 32) || !rem || !z || (n && !coeffs) || (n > 1 && !q)) return ZK_ERR_BAD_ARGS;
    zk::Fr zz, r;
    std::memcpy(&zz, z, 32);
    zk::poly_divide_host((zk::Fr*)q, &r, (const zk::Fr*)coeffs, n, zz);
    std::memcpy(rem, &r, 32);
    return ZK_OK;
  });
}

int mi355zk_fr_poly_geometry(uint32_t* run, uint32_t* tile, uint32_t* carry_width) {
  return zk::abi_guard([&]() -> int {
    if (!run || !tile || !carry_width) return ZK_ERR_BAD_ARGS;
    *run = zk::POLY_RUN;
    *tile = zk::POLY_TILE;
    *carry_width = zk::POLY_CARRY_W;
    return ZK_OK;
  });
}

}  // extern "C"
