// The R1CS evaluation of the prover: a sparse matrix x vector product over Fr, the matrix resident on the device in CSR form.
//   ProvingAssignment::enforce / eval  bellman/src/groth16/prover.rs:50-87,153-186
//     a[i] = sum over the terms of constraint i's A combination of coeff * assignment[var], likewise b and c
// plus the conversion that brings a witness to the device's number format (canonical FrRepr -> Montgomery Fr).
//
// Row lengths of real circuits are mixed: one to three terms for most constraints, ~254 for a bit decomposition, now and then thousands.
// ONE kernel, 256 rows per workgroup, two phases:
//   1. a lane walks its own row if the row has at most R1CS_SHORT_ROW_MAX terms; a longer row goes on the workgroup's list in LDS
//   2. the four waves take the listed rows in turn: 64 lanes stride the terms, a butterfly of Fr additions over the lanes ends the row
// so no lane walks a long row alone, and there is no list in device memory, no second launch and nothing to allocate.  Every add / mul
// returns the canonical residue (field.hpp), so the sum is the same bytes in any order.
//
// A BATCH of witnesses over one circuit (fr_sparse_matvec_batch_kernel) is the same kernel with R1CS_BATCH_V accumulators per lane:
// blockIdx.y names a tile of V vectors, a term's col, coeff_id and coefficient are loaded once and multiplied into V vectors, and B launches
// that do not fill the device become one grid.  V is 1 as shipped: a tile shares 8 B of index and a cached coefficient per term but costs
// 23 .. 46 VGPRs per vector, and V = 1 was the fastest at every measured size (profiles/r1cs_batch.md).  fr_r1cs_check_kernel then answers "is a * b == c in every row, and if
// not, where" for the whole batch: one ballot per wave, two atomics per wave that saw a failure.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/mi355zk.h"
#include "field.hpp"
#include "device_mem.hpp"
#include "device_util.hpp"

#ifndef R1CS_SHORT_ROW_MAX
#define R1CS_SHORT_ROW_MAX 16   // profiles/r1cs_eval.md
#endif
#ifndef R1CS_BATCH_V
#define R1CS_BATCH_V 1          // vectors per tile of the batch kernel, chosen on the clock: profiles/r1cs_batch.md
#endif

namespace zk {

// THE predicate of the satisfaction check (the kernel below and mi355zk_selftest_r1cs_check): a, b, c canonical Montgomery forms; mul
// returns the canonical residue, so a row is satisfied exactly when all eight limbs agree
ZK_HD bool r1cs_row_fails(const Fr& a, const Fr& b, const Fr& c) { return mul(a, b) != c; }

namespace {

constexpr uint32_t R1CS_WG = 256, R1CS_WAVE = 64;

__device__ __forceinline__ Fr ld(const Fr* p) {
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint4 a = q[0], b = q[1];
  Fr r;
  r.l[0] = a.x; r.l[1] = a.y; r.l[2] = a.z; r.l[3] = a.w;
  r.l[4] = b.x; r.l[5] = b.y; r.l[6] = b.z; r.l[7] = b.w;
  return r;
}
__device__ __forceinline__ void st(Fr* p, const Fr& v) {
  uint4* q = reinterpret_cast<uint4*>(p);
  q[0] = make_uint4(v.l[0], v.l[1], v.l[2], v.l[3]);
  q[1] = make_uint4(v.l[4], v.l[5], v.l[6], v.l[7]);
}

struct Csr {
  const uint32_t* row_ptr;
  const uint32_t* col;
  const uint32_t* coeff_id;
  const Fr* coeffs;
  const Fr* x;
  uint32_t n_coeffs, n_x, n_rows, nnz;
};

// the term range of row r, inside [0, nnz) whatever row_ptr holds
__device__ __forceinline__ void row_range(const Csr& m, uint32_t r, uint32_t* b, uint32_t* e) {
  const uint32_t lo = min(m.row_ptr[r], m.nnz), hi = min(m.row_ptr[r + 1], m.nnz);
  *b = lo;
  *e = max(lo, hi);
}
// acc += coeffs[coeff_id[t]] * x[col[t]] for t < nnz; an index out of range contributes nothing
__device__ __forceinline__ void add_term(const Csr& m, uint64_t t, Fr& acc) {
  const uint32_t c = m.coeff_id[t], v = m.col[t];
  if (c < m.n_coeffs && v < m.n_x) acc = add(acc, mul(ld(m.coeffs + c), ld(m.x + v)));
}

__global__ void __launch_bounds__(R1CS_WG) fr_sparse_matvec_kernel(Fr* __restrict__ out, const Csr m) {
  __shared__ uint32_t s_long[R1CS_WG];
  __shared__ uint32_t s_n_long;
  if (threadIdx.x == 0) s_n_long = 0;
  __syncthreads();
  const uint64_t row0 = (uint64_t)blockIdx.x * R1CS_WG;
  const uint64_t mine = row0 + threadIdx.x;
  if (mine < m.n_rows) {
    uint32_t b, e;
    row_range(m, (uint32_t)mine, &b, &e);
    if (e - b <= (uint32_t)R1CS_SHORT_ROW_MAX) {
      Fr acc = Fr::zero();
      for (uint64_t t = b; t < e; ++t) add_term(m, t, acc);
      st(out + mine, acc);
    } else {
      s_long[atomicAdd(&s_n_long, 1u)] = threadIdx.x;
    }
  }
  __syncthreads();
  const uint32_t n_long = s_n_long, wave = threadIdx.x / R1CS_WAVE, lane = threadIdx.x % R1CS_WAVE;
  for (uint32_t i = wave; i < n_long; i += R1CS_WG / R1CS_WAVE) {
    const uint64_t r = row0 + s_long[i];   // (< n_rows: listed by the lane that owns it)
    uint32_t b, e;
    row_range(m, (uint32_t)r, &b, &e);
    Fr acc = Fr::zero();
    for (uint64_t t = (uint64_t)b + lane; t < e; t += R1CS_WAVE) add_term(m, t, acc);
    for (uint32_t off = R1CS_WAVE / 2; off; off >>= 1) {
      Fr o;
#pragma unroll
      for (int k = 0; k < 8; ++k) o.l[k] = __shfl_xor(acc.l[k], (int)off, (int)R1CS_WAVE);
      acc = add(acc, o);
    }
    if (lane == 0) st(out + r, acc);
  }
}

// The batch: vector j of tile blockIdx.y is x + (tile V + j) x_stride, its result out + (tile V + j) out_stride.  nv = the vectors this
// tile holds (V, or fewer in the last tile): accumulator j >= nv is never loaded into, multiplied or stored.
template <int V>
__device__ __forceinline__ void add_term_batch(const Csr& m, const Fr* x, uint64_t x_stride, uint32_t nv, uint64_t t, Fr (&acc)[V]) {
  const uint32_t c = m.coeff_id[t], v = m.col[t];
  if (c < m.n_coeffs && v < m.n_x) {
    const Fr k = ld(m.coeffs + c);
#pragma unroll
    for (int j = 0; j < V; ++j)
      if ((uint32_t)j < nv) acc[j] = add(acc[j], mul(k, ld(x + j * x_stride + v)));
  }
}

template <int V>
__global__ void __launch_bounds__(R1CS_WG) fr_sparse_matvec_batch_kernel(Fr* __restrict__ out, uint64_t out_stride, const Csr m, uint64_t x_stride,
                                                                         uint32_t n_vectors) {
  __shared__ uint32_t s_long[R1CS_WG];
  __shared__ uint32_t s_n_long;
  if (threadIdx.x == 0) s_n_long = 0;
  __syncthreads();
  const uint32_t v0 = blockIdx.y * (uint32_t)V;                       // (< n_vectors: the grid has ceil(n_vectors / V) tiles)
  const uint32_t nv = min((uint32_t)V, n_vectors - v0);
  const Fr* x = m.x + (uint64_t)v0 * x_stride;
  out += (uint64_t)v0 * out_stride;
  const uint64_t row0 = (uint64_t)blockIdx.x * R1CS_WG;
  const uint64_t mine = row0 + threadIdx.x;
  if (mine < m.n_rows) {
    uint32_t b, e;
    row_range(m, (uint32_t)mine, &b, &e);
    if (e - b <= (uint32_t)R1CS_SHORT_ROW_MAX) {
      Fr acc[V];
#pragma unroll
      for (int j = 0; j < V; ++j) acc[j] = Fr::zero();
      for (uint64_t t = b; t < e; ++t) add_term_batch<V>(m, x, x_stride, nv, t, acc);
#pragma unroll
      for (int j = 0; j < V; ++j)
        if ((uint32_t)j < nv) st(out + j * out_stride + mine, acc[j]);
    } else {
      s_long[atomicAdd(&s_n_long, 1u)] = threadIdx.x;
    }
  }
  __syncthreads();
  const uint32_t n_long = s_n_long, wave = threadIdx.x / R1CS_WAVE, lane = threadIdx.x % R1CS_WAVE;
  for (uint32_t i = wave; i < n_long; i += R1CS_WG / R1CS_WAVE) {
    const uint64_t r = row0 + s_long[i];   // (< n_rows: listed by the lane that owns it)
    uint32_t b, e;
    row_range(m, (uint32_t)r, &b, &e);
    Fr acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = Fr::zero();
    for (uint64_t t = (uint64_t)b + lane; t < e; t += R1CS_WAVE) add_term_batch<V>(m, x, x_stride, nv, t, acc);
#pragma unroll
    for (int j = 0; j < V; ++j) {
      if ((uint32_t)j >= nv) break;        // (uniform over the workgroup)
      for (uint32_t off = R1CS_WAVE / 2; off; off >>= 1) {
        Fr o;
#pragma unroll
        for (int k = 0; k < 8; ++k) o.l[k] = __shfl_xor(acc[j].l[k], (int)off, (int)R1CS_WAVE);
        acc[j] = add(acc[j], o);
      }
      if (lane == 0) st(out + j * out_stride + r, acc[j]);
    }
  }
}

// Row blockIdx.x * 256 + lane of vector blockIdx.y: one ballot of the failing lanes per wave; a wave that saw one adds their number to
// n_bad[v] and offers its lowest failing row to first[v] (preset to 0xFFFFFFFF; a row index is < 2^32 - 1)
__global__ void __launch_bounds__(R1CS_WG) fr_r1cs_check_kernel(const Fr* __restrict__ a, const Fr* __restrict__ b, const Fr* __restrict__ c,
                                                                uint32_t n_rows, uint64_t vector_stride, uint32_t* first, uint32_t* n_bad) {
  const uint32_t v = blockIdx.y;
  const uint64_t row = (uint64_t)blockIdx.x * R1CS_WG + threadIdx.x;
  bool fails = false;
  if (row < n_rows) {
    const uint64_t at = (uint64_t)v * vector_stride + row;
    fails = r1cs_row_fails(ld(a + at), ld(b + at), ld(c + at));
  }
  const unsigned long long mask = __ballot(fails);                    // 64 bits: one per lane of the wave
  if (mask != 0 && threadIdx.x % R1CS_WAVE == 0) {
    atomicAdd(n_bad + v, (uint32_t)__builtin_popcountll(mask));
    atomicMin(first + v, (uint32_t)row + (uint32_t)__builtin_ctzll(mask));
  }
}

// *bad |= 1 for a row_ptr that does not go from 0 to nnz without decreasing, a col >= n_x, a coeff_id >= n_coeffs
__global__ void __launch_bounds__(256) fr_sparse_matvec_check_kernel(const uint32_t* __restrict__ row_ptr, const uint32_t* __restrict__ col,
                                                                     const uint32_t* __restrict__ coeff_id, uint32_t n_coeffs, uint32_t n_x,
                                                                     uint32_t n_rows, uint32_t nnz, uint32_t* bad) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x, first = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  bool ok = true;
  if (first == 0) ok = row_ptr[0] == 0 && row_ptr[n_rows] == nnz;
  for (uint64_t r = first; r < n_rows; r += stride) ok = ok && row_ptr[r] <= row_ptr[r + 1];
  for (uint64_t t = first; t < nnz; t += stride) ok = ok && col[t] < n_x && coeff_id[t] < n_coeffs;
  if (!ok) atomicOr(bad, 1u);
}

// out[i] = in[i] * 2^256 mod r (one Montgomery product by 2^512 mod r; out may alias in)
__global__ void __launch_bounds__(256) fr_from_repr_kernel(Fr* out, const Fr* in, uint64_t n) {
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    st(out + i, from_canonical(ld(in + i)));
}

unsigned capped_blocks(uint64_t n) {
  const uint64_t blocks = (n + 255) / 256;
  return (unsigned)(blocks > 16384 ? 16384 : blocks ? blocks : 1);
}

// the argument rules the evaluating and the checking call share (include/mi355zk.h: rc 3, before any device work)
int csr_args(const uint32_t* d_row_ptr, const uint32_t* d_col, const uint32_t* d_coeff_id, size_t n_coeffs, size_t n_x, size_t n_rows, size_t nnz) {
  const uint64_t lim = 1ull << 32;
  if (n_rows >= lim || nnz >= lim || n_x >= lim || n_coeffs >= lim) return ZK_ERR_BAD_ARGS;
  if (n_rows && !d_row_ptr) return ZK_ERR_BAD_ARGS;
  if (nnz && (!d_col || !d_coeff_id)) return ZK_ERR_BAD_ARGS;
  return ZK_OK;
}

// [base, base + ((n_vectors - 1) stride + n) 32): false if it does not fit the address space
bool strided_span(const void* base, size_t stride, size_t n_vectors, size_t n, size_t* lo, size_t* hi) {
  size_t elems, bytes;
  if (__builtin_mul_overflow(n_vectors - 1, stride, &elems) || __builtin_add_overflow(elems, n, &elems)) return false;
  if (__builtin_mul_overflow(elems, sizeof(Fr), &bytes)) return false;
  *lo = (size_t)base;
  return !__builtin_add_overflow(*lo, bytes, hi);
}

}  // namespace
}  // namespace zk

extern "C" {

int mi355zk_bn254_fr_sparse_matvec_dev(void* d_out, const uint32_t* d_row_ptr, const uint32_t* d_col, const uint32_t* d_coeff_id,
                                       const void* d_coeffs, size_t n_coeffs, const void* d_x, size_t n_x, size_t n_rows, size_t nnz, void* stream) {
  return zk::abi_guard([&]() -> int {
    if (int rc = zk::csr_args(d_row_ptr, d_col, d_coeff_id, n_coeffs, n_x, n_rows, nnz)) return rc;
    if ((n_rows && !d_out) || (n_coeffs && !d_coeffs) || (n_x && !d_x)) return ZK_ERR_BAD_ARGS;
    if (d_out && d_out == d_x) return ZK_ERR_BAD_ARGS;
    if (n_rows == 0) return ZK_OK;
    const zk::Csr m{d_row_ptr, d_col, d_coeff_id, (const zk::Fr*)d_coeffs, (const zk::Fr*)d_x,
                    (uint32_t)n_coeffs, (uint32_t)n_x, (uint32_t)n_rows, (uint32_t)nnz};
    const unsigned blocks = (unsigned)((n_rows + zk::R1CS_WG - 1) / zk::R1CS_WG);   // (< 2^24)
    hipLaunchKernelGGL(zk::fr_sparse_matvec_kernel, dim3(blocks), dim3(zk::R1CS_WG), 0, (hipStream_t)stream, (zk::Fr*)d_out, m);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
  });
}

int mi355zk_bn254_fr_sparse_matvec_batch_dev(void* d_out, size_t out_stride, const uint32_t* d_row_ptr, const uint32_t* d_col, const uint32_t* d_coeff_id,
                                             const void* d_coeffs, size_t n_coeffs, const void* d_x, size_t n_x, size_t x_stride, size_t n_vectors,
                                             size_t n_rows, size_t nnz, void* stream) {
  return zk::abi_guard([&]() -> int {
    if (int rc = zk::csr_args(d_row_ptr, d_col, d_coeff_id, n_coeffs, n_x, n_rows, nnz)) return rc;
    if ((n_rows && !d_out) || (n_coeffs && !d_coeffs) || (n_x && !d_x)) return ZK_ERR_BAD_ARGS;
    if (d_out && d_out == d_x) return ZK_ERR_BAD_ARGS;
    if (n_vectors == 0 || n_vectors > MI355ZK_R1CS_MAX_VECTORS || x_stride < n_x || out_stride < n_rows) return ZK_ERR_BAD_ARGS;
    size_t out_lo, out_hi, x_lo, x_hi;
    if (!zk::strided_span(d_out, out_stride, n_vectors, n_rows, &out_lo, &out_hi) || !zk::strided_span(d_x, x_stride, n_vectors, n_x, &x_lo, &x_hi))
      return ZK_ERR_BAD_ARGS;
    if (out_lo < x_hi && x_lo < out_hi) return ZK_ERR_BAD_ARGS;        // (an empty range overlaps nothing)
    if (n_rows == 0) return ZK_OK;
    constexpr int V = R1CS_BATCH_V;
    const zk::Csr m{d_row_ptr, d_col, d_coeff_id, (const zk::Fr*)d_coeffs, (const zk::Fr*)d_x,
                    (uint32_t)n_coeffs, (uint32_t)n_x, (uint32_t)n_rows, (uint32_t)nnz};
    const unsigned blocks = (unsigned)((n_rows + zk::R1CS_WG - 1) / zk::R1CS_WG);   // (< 2^24)
    const unsigned tiles = (unsigned)((n_vectors + V - 1) / V);                     // (< 2^16)
    hipLaunchKernelGGL(zk::fr_sparse_matvec_batch_kernel<V>, dim3(blocks, tiles), dim3(zk::R1CS_WG), 0, (hipStream_t)stream, (zk::Fr*)d_out,
                       (uint64_t)out_stride, m, (uint64_t)x_stride, (uint32_t)n_vectors);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
  });
}

int mi355zk_bn254_fr_r1cs_check_dev(const void* d_a, const void* d_b, const void* d_c, size_t n_rows, size_t vector_stride, size_t n_vectors,
                                    long long* first_bad, uint32_t* n_bad, void* stream) {
  return zk::abi_guard([&]() -> int {
    if (!first_bad || n_vectors == 0 || n_vectors > MI355ZK_R1CS_MAX_VECTORS || vector_stride < n_rows || n_rows >= (1ull << 32)) return ZK_ERR_BAD_ARGS;
    if (n_rows && (!d_a || !d_b || !d_c)) return ZK_ERR_BAD_ARGS;
    for (size_t v = 0; v < n_vectors; ++v) {
      first_bad[v] = -1;
      if (n_bad) n_bad[v] = 0;
    }
    if (n_rows == 0) return ZK_OK;
    // synchronous by contract: two words per vector of its own, as the CSR check's flag word (their free waits for the device, which this call does anyway)
    zk::DevTemp words;
    if (int rc = words.alloc(2 * n_vectors * sizeof(uint32_t))) return rc;
    uint32_t* d_first = words.as<uint32_t>();
    uint32_t* d_n_bad = d_first + n_vectors;
    std::vector<uint32_t> h(2 * n_vectors);
    hipStream_t st = (hipStream_t)stream;
    ZK_HIP(hipMemsetAsync(d_first, 0xFF, n_vectors * sizeof(uint32_t), st));
    ZK_HIP(hipMemsetAsync(d_n_bad, 0, n_vectors * sizeof(uint32_t), st));
    const unsigned blocks = (unsigned)((n_rows + zk::R1CS_WG - 1) / zk::R1CS_WG);   // (< 2^24)
    hipLaunchKernelGGL(zk::fr_r1cs_check_kernel, dim3(blocks, (unsigned)n_vectors), dim3(zk::R1CS_WG), 0, st, (const zk::Fr*)d_a, (const zk::Fr*)d_b,
                       (const zk::Fr*)d_c, (uint32_t)n_rows, (uint64_t)vector_stride, d_first, d_n_bad);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(h.data(), d_first, h.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));  // the check is done with its words: they die with this call
    for (size_t v = 0; v < n_vectors; ++v) {
      if (h[v] != 0xFFFFFFFFu) first_bad[v] = (long long)h[v];
      if (n_bad) n_bad[v] = h[n_vectors + v];
    }
    return ZK_OK;
  });
}

int mi355zk_selftest_r1cs_check(const uint64_t* a, const uint64_t* b, const uint64_t* c, size_t n_rows, long long* first_bad, uint32_t* n_bad) {
  return zk::abi_guard([&]() -> int {
    if (!first_bad || (n_rows && (!a || !b || !c)) || n_rows >= (1ull << 32)) return ZK_ERR_BAD_ARGS;
    long long first = -1;
    uint32_t count = 0;
    for (size_t i = 0; i < n_rows; ++i) {
      zk::Fr fa, fb, fc;
      std::memcpy(&fa, a + 4 * i, sizeof fa);
      std::memcpy(&fb, b + 4 * i, sizeof fb);
      std::memcpy(&fc, c + 4 * i, sizeof fc);
      if (zk::r1cs_row_fails(fa, fb, fc)) {
        if (first < 0) first = (long long)i;
        ++count;
      }
    }
    *first_bad = first;
    if (n_bad) *n_bad = count;
    return ZK_OK;
  });
}

int mi355zk_bn254_fr_sparse_matvec_check_dev(const uint32_t* d_row_ptr, const uint32_t* d_col, const uint32_t* d_coeff_id, size_t n_coeffs,
                                             size_t n_x, size_t n_rows, size_t nnz, void* stream) {
  return zk::abi_guard([&]() -> int {
    if (int rc = zk::csr_args(d_row_ptr, d_col, d_coeff_id, n_coeffs, n_x, n_rows, nnz)) return rc;
    if (!d_row_ptr) return nnz == 0 ? ZK_OK : ZK_ERR_BAD_ARGS;   // (no rows: nothing to hold a term)
    // once per matrix and synchronous by contract: a flag word of its own (its free waits for the device, which this call does anyway)
    zk::DevTemp flag;
    if (int rc = flag.alloc(sizeof(uint32_t))) return rc;
    uint32_t* d_bad = flag.as<uint32_t>();
    uint32_t bad = 1;
    hipStream_t st = (hipStream_t)stream;
    ZK_HIP(hipMemsetAsync(d_bad, 0, sizeof bad, st));
    hipLaunchKernelGGL(zk::fr_sparse_matvec_check_kernel, dim3(zk::capped_blocks(n_rows > nnz ? n_rows : nnz)), dim3(256), 0, st, d_row_ptr, d_col,
                       d_coeff_id, (uint32_t)n_coeffs, (uint32_t)n_x, (uint32_t)n_rows, (uint32_t)nnz, d_bad);
    ZK_HIP(hipGetLastError());
    ZK_HIP(hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, st));
    ZK_HIP(hipStreamSynchronize(st));  // the check is done with d_bad: it dies with this call
    return bad ? ZK_ERR_BAD_ARGS : ZK_OK;
  });
}

int mi355zk_bn254_fr_from_repr_dev(void* d_out, const void* d_in, size_t n, void* stream) {
  return zk::abi_guard([&]() -> int {
    if ((!d_out || !d_in) && n) return ZK_ERR_BAD_ARGS;
    if (n == 0) return ZK_OK;
    hipLaunchKernelGGL(zk::fr_from_repr_kernel, dim3(zk::capped_blocks(n)), dim3(256), 0, (hipStream_t)stream, (zk::Fr*)d_out, (const zk::Fr*)d_in, (uint64_t)n);
    ZK_HIP(hipGetLastError());
    return ZK_OK;
  });
}

}  // extern "C"
