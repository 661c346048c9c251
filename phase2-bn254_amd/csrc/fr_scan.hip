// Fr prefix scans on the device: running products and running sums of device-resident rows, and the scan of the ratios num[i] / den[i]
// (the grand product Z[i+1] = Z[i] num[i] / den[i] of a permutation argument, the log-derivative sum S[i+1] = S[i] + num[i] / den[i]).
//   GrandProductArgument::new  bellman/src/sonic/unhelped/grand_product_argument.rs:94-172   (c_i = a_i c_{i-1}, "serially for now" there)
// The chain is a prefix scan (fr_scan.hpp: the lane routines); it runs as reduce-then-scan in THREE launches over the run / tile shape of
// fr_poly.hip and fr_inverse.hip, and the launches are the only synchronisation between workgroups -- no flags, no look-back, no
// cooperative launch:
//   1  fr_scan_aggregate_kernel  every lane's run aggregate, a log-step scan over the lanes in LDS, one aggregate per tile
//   2  fr_scan_carry_kernel      one workgroup per ROW (blockIdx.y) scans that row's tile aggregates SCAN_CARRY_W at a time with a running
//                                carry: agg[t] becomes the aggregate of everything before tile t, and the row's total goes to d_total
//   3  fr_scan_apply_kernel      every tile reloads its runs and repeats the lane scan with its carry seeded into lane 0; every lane then
//                                chains through its run from the aggregate of everything before it and stores inclusive or exclusive values
// Rows of one tile skip launches 1 and 2.  Every lane of a tile has loaded (the barriers of the lane scan) before any lane stores, so a call
// may run in place.  Every field step returns the canonical residue, so the outputs are the serial chain's byte for byte however the
// chain is associated.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>

#include "../../include/mi355zk.h"
#include "api_internal.hpp"
#include "device_mem.hpp"
#include "fr_inverse.hpp"
#include "fr_scan.hpp"

namespace zk {
namespace {

static_assert(MI355ZK_SCAN_SUM == 1u && MI355ZK_SCAN_EXCLUSIVE == 2u, "flag bits");
constexpr size_t SCAN_MAX_ROWS = 65535;   // blockIdx.y is the row

// Inclusive scan over the 2^LOG_W lanes of the workgroup: returns (lane 0's value) o .. o (this lane's).  On return s[lane] holds every
// lane's result and all lanes have passed a barrier.
template <class Op, int LOG_W>
__device__ __forceinline__ Fr scan_lane_scan(Fr* s, Fr mine) {
  const int tid = threadIdx.x;
  s[tid] = mine;
  __syncthreads();
#pragma unroll 1
  for (int k = 0; k < LOG_W; ++k) {
    const int d = 1 << k;
    const bool has = tid >= d;
    const Fr before = s[has ? tid - d : tid];
    __syncthreads();
    if (has) {
      mine = scan_combine<Op>(before, mine);
      s[tid] = mine;
    }
    __syncthreads();
  }
  return mine;
}

template <class Op, bool HAS_NUM>
__global__ void __launch_bounds__(SCAN_WG) fr_scan_aggregate_kernel(Fr* __restrict__ agg, const Fr* __restrict__ x, uint64_t x_stride,
                                                                    const Fr* __restrict__ num, uint64_t num_stride, uint64_t n, uint32_t n_tiles) {
  __shared__ __align__(16) Fr s[SCAN_WG];
  const uint64_t lo = ((uint64_t)blockIdx.x * SCAN_WG + threadIdx.x) * SCAN_RUN;
  Fr v[SCAN_RUN];
  scan_run_load<Op>(v, x + (uint64_t)blockIdx.y * x_stride, HAS_NUM ? num + (uint64_t)blockIdx.y * num_stride : nullptr, lo, n);
  const Fr mine = scan_lane_scan<Op, SCAN_LOG_WG>(s, scan_run_aggregate<Op>(v));
  if (threadIdx.x == SCAN_WG - 1) poly_st(agg + (uint64_t)blockIdx.y * n_tiles + blockIdx.x, mine);
}

// agg: the row's n_tiles tile aggregates in, the exclusive carries out (a lane rewrites only the element it loaded)
template <class Op>
__global__ void __launch_bounds__(SCAN_CARRY_W) fr_scan_carry_kernel(Fr* __restrict__ agg, Fr* __restrict__ total, uint32_t n_tiles) {
  __shared__ __align__(16) Fr s[SCAN_CARRY_W];
  const int tid = threadIdx.x;
  Fr* A = agg + (uint64_t)blockIdx.y * n_tiles;
  Fr carry = Op::identity();   // the aggregate of the chunks before; every lane keeps the same one
#pragma unroll 1
  for (uint64_t c = 0; c * SCAN_CARRY_W < n_tiles; ++c) {
    const uint64_t tile = c * SCAN_CARRY_W + tid;
    Fr mine = tile < n_tiles ? poly_ld(A + tile) : Op::identity();
    if (tid == 0) mine = scan_combine<Op>(carry, mine);
    scan_lane_scan<Op, SCAN_LOG_CARRY>(s, mine);
    if (tile < n_tiles) poly_st(A + tile, tid ? s[tid - 1] : carry);
    carry = s[SCAN_CARRY_W - 1];
    __syncthreads();   // s is read before the next chunk's scan writes it
  }
  if (tid == 0 && total != nullptr) poly_st(total + blockIdx.y, carry);
}

// SINGLE: the row is one tile -- no carry is read, and the lane scan's last value is the row's total
template <class Op, bool HAS_NUM, bool SINGLE>
__global__ void __launch_bounds__(SCAN_WG) fr_scan_apply_kernel(Fr* out, uint64_t out_stride, const Fr* x, uint64_t x_stride, const Fr* __restrict__ num,
                                                                uint64_t num_stride, const Fr* __restrict__ carries, Fr* __restrict__ total,
                                                                uint64_t n, uint32_t n_tiles, bool exclusive) {
  __shared__ __align__(16) Fr s[SCAN_WG];
  const int tid = threadIdx.x;
  const uint64_t lo = ((uint64_t)blockIdx.x * SCAN_WG + tid) * SCAN_RUN;
  Fr v[SCAN_RUN];
  scan_run_load<Op>(v, x + (uint64_t)blockIdx.y * x_stride, HAS_NUM ? num + (uint64_t)blockIdx.y * num_stride : nullptr, lo, n);
  const Fr carry = SINGLE ? Op::identity() : poly_ld(carries + (uint64_t)blockIdx.y * n_tiles + blockIdx.x);
  Fr mine = scan_run_aggregate<Op>(v);
  if (tid == 0) mine = scan_combine<Op>(carry, mine);
  mine = scan_lane_scan<Op, SCAN_LOG_WG>(s, mine);
  if (SINGLE && total != nullptr && tid == SCAN_WG - 1) poly_st(total + blockIdx.y, mine);
  const Fr seed = tid ? s[tid - 1] : carry;
  scan_run_apply<Op>(out + (uint64_t)blockIdx.y * out_stride, v, lo, n, seed, exclusive);   // (out may be x: a lane stores only where it loaded)
}

template <class Op>
__global__ void __launch_bounds__(256) fr_scan_identity_kernel(Fr* __restrict__ total, uint32_t rows) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i < rows) poly_st(total + i, Op::identity());
}

// the tile aggregates / carries of one call: per (device, stream), under g_scan_mu from get() until the call's last launch is enqueued
// (device_mem.hpp: StreamScratch)
std::mutex g_scan_mu;
StreamScratch g_scan_scratch;

template <class Op, bool HAS_NUM>
int scan_launch(Fr* d_out, size_t out_stride, const Fr* d_in, size_t in_stride, const Fr* d_num, size_t num_stride, size_t n, size_t rows,
                bool exclusive, Fr* d_total, hipStream_t st) {
  if (n == 0 || rows == 0) {
    if (d_total != nullptr && rows) {
      hipLaunchKernelGGL(fr_scan_identity_kernel<Op>, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, st, d_total, (uint32_t)rows);
      ZK_HIP(hipGetLastError());
    }
    return ZK_OK;
  }
  const uint32_t n_tiles = (uint32_t)((n + SCAN_TILE - 1) / SCAN_TILE);
  const dim3 grid(n_tiles, (unsigned)rows);
  if (n_tiles == 1) {
    hipLaunchKernelGGL((fr_scan_apply_kernel<Op, HAS_NUM, true>), grid, dim3(SCAN_WG), 0, st, d_out, (uint64_t)out_stride, d_in, (uint64_t)in_stride, d_num,
                       (uint64_t)num_stride, (const Fr*)nullptr, d_total, (uint64_t)n, n_tiles, exclusive);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
  }
  int dev = 0;
  ZK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_scan_mu);
  void* p = nullptr;
  if (int rc = g_scan_scratch.get(dev, st, (size_t)n_tiles * rows * sizeof(Fr), &p)) return rc;
  Fr* agg = (Fr*)p;
  hipLaunchKernelGGL((fr_scan_aggregate_kernel<Op, HAS_NUM>), grid, dim3(SCAN_WG), 0, st, agg, d_in, (uint64_t)in_stride, d_num, (uint64_t)num_stride,
                     (uint64_t)n, n_tiles);
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(fr_scan_carry_kernel<Op>, dim3(1, (unsigned)rows), dim3(SCAN_CARRY_W), 0, st, agg, d_total, n_tiles);
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL((fr_scan_apply_kernel<Op, HAS_NUM, false>), grid, dim3(SCAN_WG), 0, st, d_out, (uint64_t)out_stride, d_in, (uint64_t)in_stride, d_num,
                     (uint64_t)num_stride, (const Fr*)agg, (Fr*)nullptr, (uint64_t)n, n_tiles, exclusive);
  ZK_HIP(hipGetLastError());
  return ZK_OK;
}

// [p, p + ((rows - 1) stride + n) 32): false when the range wraps the address space
bool scan_range(const void* p, size_t stride, size_t n, size_t rows, uintptr_t* lo, uintptr_t* hi) {
  if (rows > 1 && stride > ((size_t)-1 / 64) / rows) return false;
  *lo = (uintptr_t)p;
  *hi = *lo + ((rows ? rows - 1 : 0) * (rows > 1 ? stride : 0) + n) * 32;
  return *hi >= *lo;
}
bool scan_overlap(uintptr_t a_lo, uintptr_t a_hi, uintptr_t b_lo, uintptr_t b_hi) { return a_lo < b_hi && b_lo < a_hi; }

// what both device entry points refuse of one array and of the shape (include/mi355zk.h: rc 3)
bool scan_shape_ok(size_t n, size_t rows, uint32_t flags) {
  return (uint64_t)n < (1ull << 32) && rows <= SCAN_MAX_ROWS && (flags & ~(MI355ZK_SCAN_SUM | MI355ZK_SCAN_EXCLUSIVE)) == 0;
}
bool scan_stride_ok(size_t stride, size_t n, size_t rows) { return rows <= 1 || stride >= n; }

}  // namespace

int fr_scan_rows(Fr* d_out, size_t out_stride, const Fr* d_in, size_t in_stride, const Fr* d_num, size_t num_stride, size_t n, size_t rows,
                 uint32_t flags, Fr* d_total, hipStream_t st) {
  const bool ex = (flags & MI355ZK_SCAN_EXCLUSIVE) != 0;
  if (flags & MI355ZK_SCAN_SUM)
    return d_num ? scan_launch<ScanSum, true>(d_out, out_stride, d_in, in_stride, d_num, num_stride, n, rows, ex, d_total, st)
                 : scan_launch<ScanSum, false>(d_out, out_stride, d_in, in_stride, nullptr, 0, n, rows, ex, d_total, st);
  return d_num ? scan_launch<ScanProduct, true>(d_out, out_stride, d_in, in_stride, d_num, num_stride, n, rows, ex, d_total, st)
               : scan_launch<ScanProduct, false>(d_out, out_stride, d_in, in_stride, nullptr, 0, n, rows, ex, d_total, st);
}

void fr_scan_release_all() {
  std::lock_guard<std::mutex> lk(g_scan_mu);
  g_scan_scratch.release_all();
}

}  // namespace zk

extern "C" {

int mi355zk_bn254_fr_scan_dev(void* d_out, size_t out_stride, const void* d_in, size_t in_stride, size_t n, size_t rows, uint32_t flags, void* d_total,
                              void* stream) {
  return zk::abi_guard([&]() -> int {
    using namespace zk;
    if (!scan_shape_ok(n, rows, flags) || !scan_stride_ok(out_stride, n, rows) || !scan_stride_ok(in_stride, n, rows)) return ZK_ERR_BAD_ARGS;
    const bool work = n && rows;
    if (work && (!d_out || !d_in)) return ZK_ERR_BAD_ARGS;
    uintptr_t o_lo = 0, o_hi = 0, i_lo = 0, i_hi = 0, t_lo = 0, t_hi = 0;
    if (work) {
      if (!scan_range(d_out, out_stride, n, rows, &o_lo, &o_hi) || !scan_range(d_in, in_stride, n, rows, &i_lo, &i_hi)) return ZK_ERR_BAD_ARGS;
      const bool in_place = d_out == d_in && (rows == 1 || out_stride == in_stride);
      if (!in_place && scan_overlap(o_lo, o_hi, i_lo, i_hi)) return ZK_ERR_BAD_ARGS;
      if (d_total) {
        if (!scan_range(d_total, 1, 1, rows, &t_lo, &t_hi) || scan_overlap(t_lo, t_hi, o_lo, o_hi) || scan_overlap(t_lo, t_hi, i_lo, i_hi))
          return ZK_ERR_BAD_ARGS;
      }
    }
    return fr_scan_rows((Fr*)d_out, out_stride, (const Fr*)d_in, in_stride, nullptr, 0, n, rows, flags, (Fr*)d_total, (hipStream_t)stream);
  });
}

int mi355zk_bn254_fr_ratio_scan_dev(void* d_out, size_t out_stride, const void* d_num, size_t num_stride, const void* d_den, size_t den_stride, size_t n,
                                    size_t rows, uint32_t flags, void* d_total, uint32_t* d_n_zero, void* stream) {
  return zk::abi_guard([&]() -> int {
    using namespace zk;
    hipStream_t st = (hipStream_t)stream;
    if (!scan_shape_ok(n, rows, flags) || !scan_stride_ok(out_stride, n, rows) || !scan_stride_ok(den_stride, n, rows)) return ZK_ERR_BAD_ARGS;
    if (d_num && !scan_stride_ok(num_stride, n, rows)) return ZK_ERR_BAD_ARGS;
    const bool work = n && rows;
    if (work && (!d_out || !d_den)) return ZK_ERR_BAD_ARGS;
    bool copy = false;
    if (work) {
      uintptr_t o_lo, o_hi, d_lo, d_hi, x_lo, x_hi;
      if (!scan_range(d_out, out_stride, n, rows, &o_lo, &o_hi) || !scan_range(d_den, den_stride, n, rows, &d_lo, &d_hi)) return ZK_ERR_BAD_ARGS;
      copy = !(d_out == d_den && (rows == 1 || out_stride == den_stride));
      if (copy && scan_overlap(o_lo, o_hi, d_lo, d_hi)) return ZK_ERR_BAD_ARGS;
      if (d_num && (!scan_range(d_num, num_stride, n, rows, &x_lo, &x_hi) || scan_overlap(o_lo, o_hi, x_lo, x_hi))) return ZK_ERR_BAD_ARGS;
      if (d_total && (!scan_range(d_total, 1, 1, rows, &x_lo, &x_hi) || scan_overlap(o_lo, o_hi, x_lo, x_hi))) return ZK_ERR_BAD_ARGS;
    }
    if (d_n_zero) ZK_HIP(hipMemsetAsync(d_n_zero, 0, sizeof(uint32_t), st));
    if (work) {
      const size_t ostr = rows > 1 ? out_stride : n;   // (the stride of a single row is not looked at)
      if (copy) {
        if (rows == 1) ZK_HIP(hipMemcpyAsync(d_out, d_den, n * 32, hipMemcpyDeviceToDevice, st));
        else ZK_HIP(hipMemcpy2DAsync(d_out, out_stride * 32, d_den, den_stride * 32, n * 32, rows, hipMemcpyDeviceToDevice, st));
      }
      if (int rc = fr_inverse_rows((Fr*)d_out, n, ostr, rows, st, d_n_zero)) return rc;   // ONE inversion, however many rows
    }
    return fr_scan_rows((Fr*)d_out, out_stride, (const Fr*)d_out, out_stride, (const Fr*)d_num, num_stride, n, rows, flags, (Fr*)d_total, st);
  });
}

int mi355zk_selftest_fr_scan(uint64_t* out, const uint64_t* in, const uint64_t* num, size_t n, uint32_t flags, uint64_t total[4]) {
  return zk::abi_guard([&]() -> int {
    using namespace zk;
    if (!scan_shape_ok(n, 1, flags) || (n && (!out || !in))) return ZK_ERR_BAD_ARGS;
    const bool ex = (flags & MI355ZK_SCAN_EXCLUSIVE) != 0;
    const Fr t = (flags & MI355ZK_SCAN_SUM) ? scan_host<ScanSum>((Fr*)out, (const Fr*)in, (const Fr*)num, n, ex)
                                            : scan_host<ScanProduct>((Fr*)out, (const Fr*)in, (const Fr*)num, n, ex);
    if (total) std::memcpy(total, &t, 32);
    return ZK_OK;
  });
}

int mi355zk_fr_scan_geometry(uint32_t* run, uint32_t* tile, uint32_t* carry_width) {
  return zk::abi_guard([&]() -> int {
    if (!run || !tile || !carry_width) return ZK_ERR_BAD_ARGS;
    *run = zk::SCAN_RUN;
    *tile = zk::SCAN_TILE;
    *carry_width = zk::SCAN_CARRY_W;
    return ZK_OK;
  });
}

}  // extern "C"
