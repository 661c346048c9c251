// A polynomial in EVALUATION form against points: p(z) and the evaluations of (p(x) - p(z)) / (x - z) from evals[i] = p(omega^i), for many
// points per call -- the evaluation-form twin of fr_poly.hip, for a caller that holds what fr_sparse_matvec_dev and the Lagrange SRS give.
//   p(z)  = (z^n - 1)/n  sum_i f_i omega^i / (z - omega^i)          (barycentric)
//   q_i   = (f_i - p(z)) / (omega^i - z)
// Both divide by omega^i - z: ONE batch inversion (fr_inverse.hip) of the B n denominators, B the number of points.  The chain, blockIdx.y
// being the point as in fr_poly.hip:
//   0  fr_powers                 the per-call table w[i] = omega^i (n elements of scratch: read B times by steps 1, 3, 5, where recomputing a
//                                lane's power costs up to log n products per lane in each of them)
//   1  fr_evals_denominators     D[j][i] = w[i] - z_j, written where q_j will be (or into scratch when only values are asked for)
//   2  fr_inverse_rows           D <- 1 / D in place; the zero at D[j][k] of a point z_j = omega^k stays zero
//   3  fr_evals_wsum + _finish   s_j = sum_i (f_i w[i]) D[j][i];  values[j] = -(z_j^n - 1)/n s_j, or f_k for a point in the domain
//   4  fr_evals_quotient         q_j[i] = (f_i - values[j]) D[j][i]            (in the domain: q_j[k] = 0 for now)
//   5  fr_evals_wsum + _finish   points in the domain only: t_j = sum_i w[i] q_j[i], q_j[k] = -omega^-k t_j -- the x^(n-1) coefficient of a
//                                quotient of degree n - 2 is zero, and that coefficient is (1/n) sum_i q_j[i] omega^i
// The host decides per point whether z^n = 1 and finds k bit by bit (the discrete logarithm in a group of order 2^log_n); k or -1 travels by
// value with the point's constants, 32 points per launch.  Every step returns the canonical residue, so values and quotients are the unique
// field elements byte for byte whatever the order of the sums.
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

constexpr int EV_WG = 256, EV_PER_BLOCK = 2048, EV_MAX_BLOCKS = 4096;
constexpr int EV_POINTS_PER_LAUNCH = 32;   // 3.3 KB of launch arguments
struct EvalsPoint {
  Fr z;
  Fr scale;    // -(z^n - 1)/n                  (k < 0)
  Fr fix;      // -omega^-k                     (k >= 0)
  int64_t k;   // z = omega^k, or -1 for a point outside the domain
};
struct EvalsPoints {
  EvalsPoint p[EV_POINTS_PER_LAUNCH];
};

__global__ void __launch_bounds__(EV_POINTS_PER_LAUNCH) fr_evals_points_kernel(EvalsPoint* __restrict__ tab, const EvalsPoints ps, uint32_t m) {
  if (threadIdx.x < m) tab[threadIdx.x] = ps.p[threadIdx.x];
}

__global__ void __launch_bounds__(EV_WG) fr_evals_denominators_kernel(Fr* __restrict__ d, uint64_t d_stride, const Fr* __restrict__ w,
                                                                      const EvalsPoint* __restrict__ pts, uint64_t n) {
  const Fr z = pts[blockIdx.y].z;
  Fr* row = d + (uint64_t)blockIdx.y * d_stride;
  for (uint64_t i = (uint64_t)blockIdx.x * EV_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * EV_WG) poly_st(row + i, sub(poly_ld(w + i), z));
}

// the sum of the workgroup's values in s[0] after a barrier
__device__ __forceinline__ Fr evals_block_sum(Fr* s, Fr mine) {
  s[threadIdx.x] = mine;
  __syncthreads();
#pragma unroll 1
  for (int d = EV_WG / 2; d >= 1; d >>= 1) {
    if ((int)threadIdx.x < d) {
      mine = add(mine, s[threadIdx.x + d]);
      s[threadIdx.x] = mine;
    }
    __syncthreads();
  }
  return s[0];
}

// partial[j][block] = sum over the block's share of (a[i]) w[i] x_j[i]; IN_DOMAIN_ONLY: points outside the domain are skipped
template <bool HAS_A, bool IN_DOMAIN_ONLY>
__global__ void __launch_bounds__(EV_WG) fr_evals_wsum_kernel(Fr* __restrict__ partial, const Fr* __restrict__ a, const Fr* __restrict__ w,
                                                              const Fr* __restrict__ x, uint64_t x_stride, const EvalsPoint* __restrict__ pts, uint64_t n) {
  __shared__ __align__(16) Fr s[EV_WG];
  if (IN_DOMAIN_ONLY && pts[blockIdx.y].k < 0) return;   // (the whole workgroup)
  const Fr* row = x + (uint64_t)blockIdx.y * x_stride;
  Fr acc = Fr::zero();
  for (uint64_t i = (uint64_t)blockIdx.x * EV_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * EV_WG) {
    Fr t = poly_ld(w + i);
    if (HAS_A) t = mul(poly_ld(a + i), t);
    acc = add(acc, mul(t, poly_ld(row + i)));
  }
  const Fr sum = evals_block_sum(s, acc);
  if (threadIdx.x == 0) poly_st(partial + (uint64_t)blockIdx.y * gridDim.x + blockIdx.x, sum);
}

// FIX == false: values[j] = scale_j * (sum of the partials), or evals[k];  FIX == true: q_j[k] = fix_j * (sum of the partials), in-domain points only
template <bool FIX>
__global__ void __launch_bounds__(EV_WG) fr_evals_finish_kernel(Fr* __restrict__ out, uint64_t out_stride, const Fr* __restrict__ partial, uint32_t n_blocks,
                                                                const EvalsPoint* __restrict__ pts, const Fr* __restrict__ evals) {
  __shared__ __align__(16) Fr s[EV_WG];
  const EvalsPoint* pt = pts + blockIdx.y;
  const int64_t k = pt->k;
  if (FIX && k < 0) return;
  Fr acc = Fr::zero();
  for (uint32_t b = threadIdx.x; b < n_blocks; b += EV_WG) acc = add(acc, poly_ld(partial + (uint64_t)blockIdx.y * n_blocks + b));
  const Fr sum = evals_block_sum(s, acc);
  if (threadIdx.x != 0) return;
  if (FIX) poly_st(out + (uint64_t)blockIdx.y * out_stride + k, mul(pt->fix, sum));
  else poly_st(out + blockIdx.y, k >= 0 ? poly_ld(evals + k) : mul(pt->scale, sum));
}

// q_j[i] = (f_i - values[j]) * q_j[i]   (q_j holds the inverted denominators)
__global__ void __launch_bounds__(EV_WG) fr_evals_quotient_kernel(Fr* __restrict__ q, uint64_t q_stride, const Fr* __restrict__ evals,
                                                                  const Fr* __restrict__ values, uint64_t n) {
  const Fr v = poly_ld(values + blockIdx.y);
  Fr* row = q + (uint64_t)blockIdx.y * q_stride;
  for (uint64_t i = (uint64_t)blockIdx.x * EV_WG + threadIdx.x; i < n; i += (uint64_t)gridDim.x * EV_WG)
    poly_st(row + i, mul(sub(poly_ld(evals + i), v), poly_ld(row + i)));
}

// the point's constants on the host: z^n by log_n squarings; when it is one, k bit by bit -- with y = z omega^-(the bits found so far), bit b
// is set exactly when y^(2^(log_n - 1 - b)) is not one (it is then -1), and y loses that bit by a product with omega^-(2^b)
EvalsPoint evals_point(const Fr& z, uint32_t log_n, const Fr& omegainv, const Fr& ninv) {
  EvalsPoint pt;
  pt.z = z;
  pt.scale = pt.fix = Fr::zero();
  pt.k = -1;
  const Fr one = Fr::one();
  Fr zn = z;
  for (uint32_t i = 0; i < log_n; ++i) zn = sqr(zn);
  if (zn != one) {
    pt.scale = neg(mul(sub(zn, one), ninv));
    return pt;
  }
  Fr y = z, step = omegainv, shed = one;   // step = omega^-(2^b), shed = omega^-k so far
  int64_t k = 0;
  for (uint32_t b = 0; b < log_n; ++b) {
    Fr t = y;
    for (uint32_t i = b + 1; i < log_n; ++i) t = sqr(t);
    if (t != one) {
      k |= (int64_t)1 << b;
      y = mul(y, step);
      shed = mul(shed, step);
    }
    step = sqr(step);
  }
  pt.k = k;
  pt.fix = neg(shed);
  return pt;
}

std::mutex g_evals_mu;
StreamScratch g_evals_scratch;

unsigned evals_blocks(uint64_t n) {
  const uint64_t b = (n + EV_PER_BLOCK - 1) / EV_PER_BLOCK;
  return (unsigned)(b > (uint64_t)EV_MAX_BLOCKS ? (uint64_t)EV_MAX_BLOCKS : b);
}

// d_q == nullptr: values only.  The arguments have been checked.
int evals_run(Fr* d_q, size_t q_stride, Fr* d_values, const Fr* d_evals, uint32_t log_n, const uint64_t* z, size_t n_points, hipStream_t st) {
  const uint64_t n = 1ull << log_n;
  Fr omega, omegainv, ninv;
  if (int rc = mi355zk_bn254_fr_domain_constants(log_n, (uint64_t*)&omega, (uint64_t*)&omegainv, nullptr, (uint64_t*)&ninv)) return rc;
  std::vector<EvalsPoint> pts(n_points);
  bool any_in_domain = false;
  for (size_t j = 0; j < n_points; ++j) {
    Fr zz;
    std::memcpy(&zz, z + 4 * j, 32);
    pts[j] = evals_point(zz, log_n, omegainv, ninv);
    any_in_domain |= pts[j].k >= 0;
  }
  const unsigned n_blocks = evals_blocks(n);
  const size_t tab_bytes = (n_points * sizeof(EvalsPoint) + 255) & ~(size_t)255;
  const size_t w_bytes = n * sizeof(Fr), part_bytes = n_points * (size_t)n_blocks * sizeof(Fr);
  const size_t d_bytes = d_q ? 0 : n_points * n * sizeof(Fr);
  int dev = 0;
  ZK_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lk(g_evals_mu);
  void* p = nullptr;
  if (int rc = g_evals_scratch.get(dev, st, tab_bytes + w_bytes + part_bytes + d_bytes, &p)) return rc;
  EvalsPoint* tab = (EvalsPoint*)p;
  Fr* w = (Fr*)((char*)p + tab_bytes);
  Fr* partial = w + n;
  Fr* d = d_q ? d_q : partial + n_points * (size_t)n_blocks;
  const size_t d_stride = d_q ? q_stride : (size_t)n;
  EvalsPoints ps;
  for (size_t p0 = 0; p0 < n_points; p0 += EV_POINTS_PER_LAUNCH) {
    const size_t m = n_points - p0 < (size_t)EV_POINTS_PER_LAUNCH ? n_points - p0 : (size_t)EV_POINTS_PER_LAUNCH;
    std::memcpy(ps.p, pts.data() + p0, m * sizeof(EvalsPoint));
    hipLaunchKernelGGL(fr_evals_points_kernel, dim3(1), dim3(EV_POINTS_PER_LAUNCH), 0, st, tab + p0, ps, (uint32_t)m);
  }
  ZK_HIP(hipGetLastError());
  if (int rc = fr_powers(w, omega, Fr::one(), n, st)) return rc;
  const dim3 grid(n_blocks, (unsigned)n_points), one_block(1, (unsigned)n_points);
  hipLaunchKernelGGL(fr_evals_denominators_kernel, grid, dim3(EV_WG), 0, st, d, (uint64_t)d_stride, (const Fr*)w, (const EvalsPoint*)tab, n);
  ZK_HIP(hipGetLastError());
  if (int rc = fr_inverse_rows(d, n, d_stride, n_points, st)) return rc;
  hipLaunchKernelGGL((fr_evals_wsum_kernel<true, false>), grid, dim3(EV_WG), 0, st, partial, d_evals, (const Fr*)w, (const Fr*)d, (uint64_t)d_stride,
                     (const EvalsPoint*)tab, n);
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(fr_evals_finish_kernel<false>, one_block, dim3(EV_WG), 0, st, d_values, (uint64_t)0, (const Fr*)partial, (uint32_t)n_blocks,
                     (const EvalsPoint*)tab, d_evals);
  ZK_HIP(hipGetLastError());
  if (d_q == nullptr) return ZK_OK;
  hipLaunchKernelGGL(fr_evals_quotient_kernel, grid, dim3(EV_WG), 0, st, d_q, (uint64_t)q_stride, d_evals, (const Fr*)d_values, n);
  ZK_HIP(hipGetLastError());
  if (!any_in_domain) return ZK_OK;
  hipLaunchKernelGGL((fr_evals_wsum_kernel<false, true>), grid, dim3(EV_WG), 0, st, partial, (const Fr*)nullptr, (const Fr*)w, (const Fr*)d_q,
                     (uint64_t)q_stride, (const EvalsPoint*)tab, n);
  ZK_HIP(hipGetLastError());
  hipLaunchKernelGGL(fr_evals_finish_kernel<true>, one_block, dim3(EV_WG), 0, st, d_q, (uint64_t)q_stride, (const Fr*)partial, (uint32_t)n_blocks,
                     (const EvalsPoint*)tab, (const Fr*)nullptr);
  ZK_HIP(hipGetLastError());
  return ZK_OK;
}

bool ranges_overlap(uintptr_t a_lo, uintptr_t a_hi, uintptr_t b_lo, uintptr_t b_hi) { return a_lo < b_hi && b_lo < a_hi; }

}  // namespace

void fr_evals_release_all() {
  std::lock_guard<std::mutex> lk(g_evals_mu);
  g_evals_scratch.release_all();
}

}  // namespace zk

extern "C" {

int mi355zk_bn254_fr_evals_divide_dev(void* d_q, size_t q_stride, void* d_values, const void* d_evals, uint32_t log_n, const uint64_t* z,
                                      size_t n_points, void* stream) {
  return zk::abi_guard([&]() -> int {
    if (!d_evals || !d_values || !z || log_n > 28 || n_points == 0 || n_points > MI355ZK_POLY_MAX_POINTS) return ZK_ERR_BAD_ARGS;
    const size_t n = (size_t)1 << log_n;
    if (d_q) {
      if (q_stride < n || q_stride > ((size_t)-1 / 64) / n_points) return ZK_ERR_BAD_ARGS;   // (the quotient range would wrap the address space)
      const uintptr_t q_lo = (uintptr_t)d_q, q_hi = q_lo + ((n_points - 1) * q_stride + n) * 32;
      const uintptr_t e_lo = (uintptr_t)d_evals, v_lo = (uintptr_t)d_values;
      if (q_hi < q_lo || zk::ranges_overlap(q_lo, q_hi, e_lo, e_lo + n * 32) || zk::ranges_overlap(q_lo, q_hi, v_lo, v_lo + n_points * 32))
        return ZK_ERR_BAD_ARGS;
    }
    return zk::evals_run((zk::Fr*)d_q, q_stride, (zk::Fr*)d_values, (const zk::Fr*)d_evals, log_n, z, n_points, (hipStream_t)stream);
  });
}

}  // extern "C"
