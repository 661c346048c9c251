// The host-buffer entry points that share nothing with the multiexp (host_entry.hip) but the lease of host_pools.hpp: batch_exp, dense_multiexp /
// merge_pairs, the NTT and the H polynomial, and the QAP sparse matvec (device-resident and host-buffer forms, with its CSR check kernel).
// Their cut arithmetic is host_plan.hpp's; the extern "C" wrappers are api.hip's.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "../../include/mi355zk.h"
#include "curveu.hpp"
#include "api_internal.hpp"
#include "host_plan.hpp"
#include "host_pools.hpp"

namespace zk {
// ------------------------------------------------------------------------------------------------
// batch_exp on HOST buffers, over the device set: what `MPCParameters::contribute` (phase2/src/parameters.rs:423-470: every point of L
// and H times delta^-1) and powersoftau's `batch_exp` (batched_accumulator.rs:1130-1181) are to a single-process caller.  The points are
// independent, so they shard by CONTIGUOUS POINT RANGE with no exchange at all (shard.batch_exp_sharded is the
// one-process-per-GPU form): device d of mi355zk_init's set takes range d -- upload, the batch_exp kernels, download -- from its own
// host thread; with one device the whole vector is one range.  Ranges are worked off in pieces of 2^18 points (a piece's buffers
// come from the grow-only pool, so a 2^26-point vector does not allocate 10 GiB).  g2_trusted: the promise flag of batch_exp_dev.
template <class F>
int batch_exp_host(uint8_t* out, const uint8_t* bases, const uint64_t* scalars, size_t n, int same_scalar, bool g2_trusted) {
  if ((n && (!out || !bases)) || !scalars) return ZK_ERR_BAD_ARGS;
  if (n == 0) return ZK_OK;
  if (n >= (1ull << 31)) return ZK_ERR_BAD_ARGS;
  constexpr size_t rec = sizeof(Affine<F>);
  std::vector<int> devs;
  if (int rc = devset_or_current(&devs)) return rc;
  const size_t parts = range_parts(n, devs.size(), 1024);
  auto run_range = [&](size_t d) -> int {
    const size_t lo = n * d / parts, hi = n * (d + 1) / parts;
    if (hipSetDevice(devs[d]) != hipSuccess) return ZK_ERR_DEVICE;
    // pieces of 2^18 points, double-buffered
    const size_t piece = (size_t)1 << 18;
    const size_t m_max = hi - lo < piece ? hi - lo : piece;
    const size_t in_bytes = (m_max * rec + 255) & ~(size_t)255;
    const size_t sc_bytes = same_scalar ? 256 : ((m_max * 32 + 255) & ~(size_t)255);
    Events ev(4);   // (declared before the lease: destroyed after both streams are idle)
    hipEvent_t* up = &ev.e[0];
    hipEvent_t* done = &ev.e[2];
    CallLease lease;
    int rc = lease.open(devs[d], 4 * in_bytes + 2 * sc_bytes);
    if (rc) return rc;
    HostStage* S = lease.S;
    char* base = (char*)lease.buf;
    char* d_in[2] = {base, base + in_bytes};
    char* d_out[2] = {base + 2 * in_bytes, base + 3 * in_bytes};
    char* d_sc[2] = {base + 4 * in_bytes, base + 4 * in_bytes + sc_bytes};
    auto fail = [&](hipError_t e) {
      std::fprintf(stderr, "[mi355zk] batch_exp (host buffers): HIP error %d (%s)\n", (int)e, hipGetErrorString(e));
      return ZK_ERR_DEVICE;
    };
    hipError_t e = ev.create();
    if (e != hipSuccess) return fail(e);
    if (same_scalar && (e = hipMemcpyAsync(d_sc[0], scalars, 32, hipMemcpyHostToDevice, S->copy)) != hipSuccess) return fail(e);
    // ONE host thread keeps the device busy although copies from / to PAGEABLE host memory block it: the kernels of piece i + 1 are
    // always queued before the thread waits for piece i's download, and piece i + 2 is uploaded (into the buffer piece i's kernels
    // have finished with: its download has just returned) while piece i + 1 computes.
    const size_t n_pieces = (hi - lo + piece - 1) / piece;
    auto upload_and_launch = [&](size_t i) -> bool {   // false: rc, or else e, says why
      const size_t p0 = lo + i * piece, m = hi - p0 < piece ? hi - p0 : piece;
      const int k = (int)(i & 1);
      if ((e = hipMemcpyAsync(d_in[k], bases + p0 * rec, m * rec, hipMemcpyHostToDevice, S->copy)) != hipSuccess) return false;
      if (!same_scalar && (e = hipMemcpyAsync(d_sc[k], scalars + p0 * 4, m * 32, hipMemcpyHostToDevice, S->copy)) != hipSuccess) return false;
      if ((e = hipEventRecord(up[k], S->copy)) != hipSuccess || (e = hipStreamWaitEvent(S->compute, up[k], 0)) != hipSuccess) return false;
      rc = batch_exp<F>(d_out[k], d_in[k], 0, same_scalar ? d_sc[0] : d_sc[k], same_scalar, m, (void*)S->compute, nullptr, false, g2_trusted);
      if (rc) return false;
      return (e = hipEventRecord(done[k], S->compute)) == hipSuccess;
    };
    for (size_t i = 0; i < 2 && i < n_pieces; ++i)
      if (!upload_and_launch(i)) return rc ? rc : fail(e);
    for (size_t i = 0; i < n_pieces; ++i) {
      const size_t p0 = lo + i * piece, m = hi - p0 < piece ? hi - p0 : piece;
      const int k = (int)(i & 1);
      if ((e = hipStreamWaitEvent(S->copy, done[k], 0)) != hipSuccess) return fail(e);
      if ((e = hipMemcpyAsync(out + p0 * rec, d_out[k], m * rec, hipMemcpyDeviceToHost, S->copy)) != hipSuccess) return fail(e);
      if ((e = hipStreamSynchronize(S->copy)) != hipSuccess) return fail(e);   // piece i is on the host; its buffers are free
      if (i + 2 < n_pieces && !upload_and_launch(i + 2)) return rc ? rc : fail(e);
    }
    if ((e = hipStreamSynchronize(S->compute)) != hipSuccess) return fail(e);
    return ZK_OK;
  };
  return first_error(fan_out(parts, run_range));
}

// ------------------------------------------------------------------------------------------------
// dense_multiexp / merge_pairs on HOST buffers, over the device set: the verification multiexps of the ceremony code (SURVEY 8f row 2:
// powersoftau/src/utils.rs:112-135, 189-292; phase2/src/utils.rs:59-105) for a single-process caller.  sum_i rho_i * v_i is linear in the
// points, so the vectors are cut into pieces of 2^22 points, every piece is one device call (msm_g*_dense_device: digits and partition
// shared by the two sums of merge_pairs) and the Jacobian partials are added on the host.  The pieces are dealt to TWO host threads per
// device of mi355zk_init's set (one piece uploads -- pageable copies block their thread -- while the other computes); v2 == nullptr:
// dense_multiexp.  No Source errors (infinity bases add nothing: the reference's dense contract).
template <int GROUP>
int dense_host(const uint8_t* v1, const uint8_t* v2, const uint64_t* rho, size_t n, uint64_t* out_s, uint64_t* out_sx, const FrRandomStream* rnd) {
  using J = typename std::conditional<GROUP == 1, G1Jacobian, G2Jacobian>::type;
  constexpr size_t rec = GROUP == 1 ? 64 : 128;
  if (!out_s || (v2 && !out_sx) || (n && (!v1 || (!rho && !rnd))) || n >= (1ull << 31)) return ZK_ERR_BAD_ARGS;
  J total = J::zero(), total2 = J::zero();
  if (n > 0) {
    std::vector<int> devs;
    if (int rc = devset_or_current(&devs)) return rc;
    const size_t piece = host_knobs().dense_piece;
    const size_t n_pieces = (n + piece - 1) / piece;
    size_t workers = 2 * devs.size();
    if (workers > n_pieces) workers = n_pieces;
    struct Part { J s, sx; };
    std::vector<Part> parts(workers);
    for (auto& pt : parts) { pt.s = J::zero(); pt.sx = J::zero(); }
    std::atomic<size_t> next{0};
    // (a worker takes pieces until none is left: one that got no thread and runs late, on the calling thread, finds nothing to do)
    auto work = [&](size_t wk) -> int {
      Part& P = parts[wk];
      const int dev = devs[wk % devs.size()];
      if (next.load() >= n_pieces) return ZK_OK;   // (run late: no stage, no buffer for nothing)
      if (hipSetDevice(dev) != hipSuccess) return ZK_ERR_DEVICE;
      const size_t m_max = n < piece ? n : piece;
      const size_t vb = ((m_max + 16) * rec + 255) & ~(size_t)255;
      CallLease lease;
      if (int rc = lease.open(dev, (v2 ? 2 : 1) * vb + m_max * 32)) return rc;
      HostStage* S = lease.S;
      char* d_v1 = (char*)lease.buf;
      const size_t shift = shared_shift(v1, v2, rec, n);   // power_pairs: v2 a few records into v1 shares v1's upload
      const bool shared = shift != (size_t)-1;
      char* d_v2 = v2 ? (shared ? d_v1 + shift * rec : d_v1 + vb) : nullptr;
      char* d_rho = d_v1 + (v2 ? 2 : 1) * vb;
      for (;;) {
        const size_t i = next.fetch_add(1);
        if (i >= n_pieces) break;
        const size_t p0 = i * piece, m = n - p0 < piece ? n - p0 : piece;
        hipError_t e = hipMemcpyAsync(d_v1, v1 + p0 * rec, (m + (shared ? shift : 0)) * rec, hipMemcpyHostToDevice, S->compute);
        if (e == hipSuccess && v2 && !shared) e = hipMemcpyAsync(d_v2, v2 + p0 * rec, m * rec, hipMemcpyHostToDevice, S->compute);
        if (e == hipSuccess && !rnd) e = hipMemcpyAsync(d_rho, rho + p0 * 4, m * 32, hipMemcpyHostToDevice, S->compute);
        if (e != hipSuccess) {
          std::fprintf(stderr, "[mi355zk] dense multiexp (host buffers): HIP error %d (%s)\n", (int)e, hipGetErrorString(e));
          return ZK_ERR_DEVICE;
        }
        // (no upload of exponents: scalars p0 .. p0 + m - 1 of the caller's stream, whatever the piece size and whichever device runs the piece)
        if (rnd)
          if (int rc = fr_random_fill(d_rho, m, rnd->key, rnd->stream_id, p0, S->compute)) return rc;
        J a = J::zero(), b = J::zero();
        const int rc = GROUP == 1 ? msm_g1_dense_device(d_v1, d_v2, d_rho, m, S->compute, reinterpret_cast<uint64_t*>(&a), v2 ? reinterpret_cast<uint64_t*>(&b) : nullptr)
                                  : msm_g2_dense_device(d_v1, d_v2, d_rho, m, S->compute, reinterpret_cast<uint64_t*>(&a), v2 ? reinterpret_cast<uint64_t*>(&b) : nullptr);
        if (rc != ZK_OK) return rc;
        jac_add(P.s, a);
        if (v2) jac_add(P.sx, b);
      }
      return ZK_OK;
    };
    if (int rc = first_error(fan_out(workers, work))) return rc;
    for (auto& pt : parts) {
      jac_add(total, pt.s);
      if (v2) jac_add(total2, pt.sx);
    }
  }
  std::memcpy(out_s, &total, sizeof total);
  if (v2) std::memcpy(out_sx, &total2, sizeof total2);
  return ZK_OK;
}

// best_fft / the domain operations on a HOST array (what a bellman shim calls with `&mut [Scalar<E>]`): upload, transform in place
// on the device, copy back.  Device buffer and stream are leased from the pools of the host-buffer entry points -- round 2
// hipMalloc'ed and hipFree'd per call (both synchronise the whole device, i.e. every other thread's multiexp) and ran on the null
// stream.  `a` is written by the final copy only: on a device failure (rc < 0) the caller's array is untouched and it can fall
// back to its own serial_fft.
int ntt_host(uint64_t* a, uint32_t log_n, int op, const uint64_t* omega) {
  if (!a) return ZK_ERR_BAD_ARGS;
  if (log_n > 28) return ZK_ERR_BAD_ARGS;
  const size_t bytes = (size_t)32 << log_n;
  int dev = 0;
  ZK_HIP(hipGetDevice(&dev));
  CallLease lease;   // (the lease synchronises the streams before the buffer is handed on)
  int rc = lease.open(dev, bytes);
  if (rc) return rc;
  HostStage* S = lease.S;
  void* d = lease.buf;
  ZK_HIP(hipMemcpyAsync(d, a, bytes, hipMemcpyHostToDevice, S->compute));
  if (omega) {
    Fr w;
    std::memcpy(&w, omega, 32);
    rc = ntt_run((Fr*)d, log_n, w, S->compute);
  } else {
    rc = domain_op_dev((Fr*)d, log_n, op, S->compute);
  }
  if (rc != ZK_OK) return rc;
  ZK_HIP(hipStreamSynchronize(S->compute));  // a failed kernel surfaces here, before the caller's array is touched
  ZK_HIP(hipMemcpyAsync(a, d, bytes, hipMemcpyDeviceToHost, S->compute));
  ZK_HIP(hipStreamSynchronize(S->compute));
  return ZK_OK;
}

// The prover's H polynomial (prover.rs:216-248) from three HOST arrays: one upload of a, b and c, the chain in HBM, one download of
// h -- 128 B per element over the link where seven ntt_host calls move 448 B.  The arrays travel one after the other on the copy
// stream, in pieces of H_POLY_PIECE elements (what the runtime's pinned staging holds per hop -- the streamed multiexp's uploads go
// the same way), and an array's ifft and coset_fft are queued on the compute stream behind the event that ends its upload: they run
// while the next array crosses the link, so that only c's two transforms, the combine and the icoset_fft are exposed behind the last
// byte.  (Pipelined single transforms rather than the batched launches of the device entry behind the last upload: measured on one box,
// profiles/h_poly.md -- 2^20 3.14-3.28 ms against 3.52-3.54 ms; 2^16 0.40-0.45 against 0.37-0.39, inside that size's run-to-run spread.)
// The inputs are only read; h is written by the
// final copy only.  Buffer, streams: the pools of the host-buffer entry points; three events per call, as msm_host_run makes its own.
constexpr size_t H_POLY_PIECE = (size_t)1 << 17;   // elements per copy (4 MiB)
int h_poly_host(uint64_t* h, const uint64_t* a, const uint64_t* b, const uint64_t* c, size_t len, uint32_t log_n, uint32_t flags) {
  const size_t n = (size_t)1 << log_n, bytes = n * 32;
  int dev = 0;
  ZK_HIP(hipGetDevice(&dev));
  Events ev(3);   // (declared before the lease: destroyed after both streams are idle)
  CallLease lease;
  int rc = lease.open(dev, 3 * bytes);
  if (rc) return rc;
  HostStage* S = lease.S;
  ZK_HIP(ev.create());
  Fr* d[3] = {(Fr*)lease.buf, (Fr*)lease.buf + n, (Fr*)lease.buf + 2 * n};
  const uint64_t* src[3] = {a, b, c};
  for (int k = 0; k < 3; ++k) {
    if (len < n) ZK_HIP(hipMemsetAsync(d[k] + len, 0, (n - len) * 32, S->copy));   // from_coeffs: resize(m, zero) (domain.rs:80-82)
    for (size_t lo = 0; lo < len; lo += H_POLY_PIECE) {
      const size_t m = len - lo < H_POLY_PIECE ? len - lo : H_POLY_PIECE;
      ZK_HIP(hipMemcpyAsync(d[k] + lo, src[k] + lo * 4, m * 32, hipMemcpyHostToDevice, S->copy));
    }
    ZK_HIP(hipEventRecord(ev[k], S->copy));
    ZK_HIP(hipStreamWaitEvent(S->compute, ev[k], 0));
#ifndef ZK_H_POLY_HOST_BATCHED
    rc = domain_op_dev(d[k], log_n, MI355ZK_OP_IFFT, S->compute);
    if (rc == ZK_OK) rc = domain_op_dev(d[k], log_n, MI355ZK_OP_COSET_FFT, S->compute);
    if (rc != ZK_OK) return rc;
#endif
  }
#ifdef ZK_H_POLY_HOST_BATCHED   // (the variant the pipelined form was measured against: tools/build_variant.sh, profiles/h_poly.md)
  rc = domain_op_batch_dev(d, 3, log_n, MI355ZK_OP_IFFT, S->compute);
  if (rc == ZK_OK) rc = domain_op_batch_dev(d, 3, log_n, MI355ZK_OP_COSET_FFT, S->compute);
  if (rc != ZK_OK) return rc;
#endif
  rc = h_poly_finish_dev(d[0], d[1], d[2], log_n, flags, S->compute);
  if (rc != ZK_OK) return rc;
  ZK_HIP(hipStreamSynchronize(S->compute));  // a failed kernel surfaces here
  if (n > 1) {
    ZK_HIP(hipMemcpyAsync(h, d[0], (n - 1) * 32, hipMemcpyDeviceToHost, S->compute));   // the last coefficient is dropped (prover.rs:243-246)
    ZK_HIP(hipStreamSynchronize(S->compute));
  }
  return ZK_OK;
}


// out[r] = sum_{t in [row_ptr[r], row_ptr[r+1])} coeff[t] * bases[col[t]], affine (QAP evaluation, parameters.rs:225-294)
// CSR sanity on the device: flag |= 1 if some col[t] >= n_bases, |= 2 if row_ptr is not 0 = row_ptr[0] <= ... <= row_ptr[n_rows] = nnz
__global__ void __launch_bounds__(256) csr_check_kernel(const uint32_t* __restrict__ row_ptr, const uint32_t* __restrict__ col, uint64_t n_rows,
                                                       uint64_t nnz, uint64_t n_bases, uint32_t* __restrict__ flag) {
  const uint64_t stride = (uint64_t)gridDim.x * blockDim.x;
  uint32_t bad = 0;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < nnz; t += stride)
    if (col[t] >= n_bases) bad |= 1u;
  for (uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; r <= n_rows; r += stride) {
    const uint32_t v = row_ptr[r];
    if ((r == 0 && v != 0) || (r == n_rows && v != nnz) || (r < n_rows && v > row_ptr[r + 1])) bad |= 2u;
  }
  if (bad) atomicOr(flag, bad);
}

template <class F>
int sparse_matvec(void* d_out, const void* d_bases, size_t n_bases, const uint32_t* d_row_ptr, const uint32_t* d_col, const void* d_coeffs,
                         size_t n_rows, size_t nnz, void* stream, int group, bool g2_trusted, void* d_scratch, size_t scratch_bytes) {
  // d_scratch: the caller's buffer for the term products (the host-buffer form leases it with its other buffers: hipMalloc / hipFree per
  // call synchronise the whole device, i.e. every other thread's multiexp): room for the terms, 256 B of flags and one byte per base
  if (!d_out || !d_row_ptr || (nnz && (!d_bases || !d_col || !d_coeffs)) || n_rows >= (1ull << 31) || nnz >= (1ull << 31)) return ZK_ERR_BAD_ARGS;
  if (n_rows == 0) return ZK_OK;
  // G2 without the caller's promise: when the bases are reused (nnz >= 2 n_bases: a circuit has ~3 terms per Lagrange coefficient), ONE
  // membership test per base (psi(P) == mu P: 127 doublings + 68 additions) buys the psi split (a third fewer operations) and the
  // r - 1 shortcut for every term of a member, and only the terms of the other bases take the plain windows -- the result is the
  // reference's either way.  (2^20 bases, 2.9 M terms: 156 -> ~155 ms general coefficients, 90 -> ~61 ms with 90 % unit coefficients.)
  const bool by_member = std::is_same<F, Fq2>::value && !g2_trusted && nnz >= 2 * n_bases && n_bases > 0;
  const size_t terms_bytes = ((nnz ? nnz : 1) * sizeof(Affine<F>) + 255) & ~(size_t)255;
  DevTemp own;  // (used when the caller brought no scratch, or too little)
  const size_t need = terms_bytes + 256 + (by_member ? n_bases : 0);
  if (d_scratch == nullptr || scratch_bytes < need) {
    if (int rc = own.alloc(need)) return rc;
    d_scratch = own.p;
  }
  Affine<F>* d_terms = (Affine<F>*)d_scratch;
  uint8_t* d_member = by_member ? reinterpret_cast<uint8_t*>(d_terms) + terms_bytes + 256 : nullptr;
  {
    // the ABI cannot trust the index arrays: an out-of-range column would be an out-of-bounds gather in batch_exp
    uint32_t* d_flag = reinterpret_cast<uint32_t*>(reinterpret_cast<char*>(d_terms) + terms_bytes);
    uint32_t h_flag = 0;
    ZK_HIP(hipMemsetAsync(d_flag, 0, 4, (hipStream_t)stream));
    const uint64_t work = nnz > n_rows + 1 ? nnz : n_rows + 1;
    hipLaunchKernelGGL(csr_check_kernel, dim3((unsigned)((work + 255) / 256 < 4096 ? (work + 255) / 256 : 4096)), dim3(256), 0, (hipStream_t)stream,
                       d_row_ptr, d_col, (uint64_t)n_rows, (uint64_t)nnz, (uint64_t)n_bases, d_flag);
    ZK_HIP(hipMemcpyAsync(&h_flag, d_flag, 4, hipMemcpyDeviceToHost, (hipStream_t)stream));
    ZK_HIP(hipStreamSynchronize((hipStream_t)stream));
    if (h_flag) return ZK_ERR_BAD_ARGS;
  }
  if constexpr (std::is_same<F, Fq2>::value)
    if (by_member)
      if (int rc = g2_subgroup_flags(d_bases, n_bases, stream, d_member)) return rc;
  if (int rc = batch_exp<F>(d_terms, d_bases, 0, d_coeffs, 0, nnz, stream, d_col, /*shortcut_unit_scalars=*/true, g2_trusted, d_member)) return rc;
  // the segmented sum synchronises the stream before it returns (msm_host.hpp: segsum_device): nothing queued reads `own` when it dies
  return group == 1 ? segsum_g1_device(d_terms, nnz, d_row_ptr, (uint32_t)n_rows, (hipStream_t)stream, d_out)
                    : segsum_g2_device(d_terms, nnz, d_row_ptr, (uint32_t)n_rows, (hipStream_t)stream, d_out);
}

// The QAP evaluation on HOST buffers, over the device set (SURVEY 8f row 3 for a single-process caller: MPCParameters::new over a
// 2^20+-constraint circuit): the rows of the CSR matrix are independent, so device d takes the d-th contiguous ROW range -- its slice of
// (col, coeff), a row_ptr rebased to zero, and the WHOLE base vector (any row may name any Lagrange coefficient) -- and writes its rows
// of the output; no exchange.  The index arrays are validated on the device as in the _dev form; row_ptr[0] == 0, row_ptr[n_rows] == nnz
// and monotonicity across the cuts are checked here.
template <class F>
int sparse_matvec_host(uint8_t* out, const uint8_t* bases, size_t n_bases, const uint32_t* row_ptr, const uint32_t* col, const uint64_t* coeffs,
                              size_t n_rows, size_t nnz, int group, bool g2_trusted) {
  constexpr size_t rec = sizeof(Affine<F>);
  if (!row_ptr || (n_rows && !out) || (nnz && (!bases || !col || !coeffs)) || n_rows >= (1ull << 31) || nnz >= (1ull << 31) || n_bases >= (1ull << 31)) return ZK_ERR_BAD_ARGS;
  if (n_rows == 0) return ZK_OK;
  if (row_ptr[0] != 0 || row_ptr[n_rows] != nnz) return ZK_ERR_BAD_ARGS;
  std::vector<int> devs;
  if (int rc = devset_or_current(&devs)) return rc;
  const size_t parts = range_parts(n_rows, devs.size(), 128);
  const std::vector<size_t> cut = weight_cuts(row_ptr, n_rows, nnz, parts);   // (equal rows + terms per device)
  auto run_range = [&](size_t d) -> int {
    const size_t r0 = cut[d], r1 = cut[d + 1];
    if (r1 == r0) return ZK_OK;
    const uint32_t t0 = row_ptr[r0], t1 = row_ptr[r1];
    if (t1 < t0) return ZK_ERR_BAD_ARGS;
    const size_t rows = r1 - r0, terms = t1 - t0;
    if (hipSetDevice(devs[d]) != hipSuccess) return ZK_ERR_DEVICE;
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };
    const size_t o_bases = 0, o_out = o_bases + al((n_bases ? n_bases : 1) * rec), o_rp = o_out + al(rows * rec), o_col = o_rp + al((rows + 1) * 4),
                 o_cf = o_col + al((terms ? terms : 1) * 4), o_scr = o_cf + al((terms ? terms : 1) * 32),
                 scr_bytes = al((terms ? terms : 1) * rec) + 256 + al(n_bases), total = o_scr + scr_bytes;
    CallLease lease;
    if (int rc = lease.open(devs[d], total)) return rc;
    HostStage* S = lease.S;
    char* base = (char*)lease.buf;
    std::vector<uint32_t> rp(rows + 1);
    for (size_t r = 0; r <= rows; ++r) {
      const uint32_t v = row_ptr[r0 + r];
      if (v < t0 || v > t1) return ZK_ERR_BAD_ARGS;   // (monotone inside the range is checked on the device)
      rp[r] = v - t0;
    }
    hipError_t e = hipSuccess;
    if (n_bases) e = hipMemcpyAsync(base + o_bases, bases, n_bases * rec, hipMemcpyHostToDevice, S->compute);
    if (e == hipSuccess) e = hipMemcpyAsync(base + o_rp, rp.data(), (rows + 1) * 4, hipMemcpyHostToDevice, S->compute);
    if (e == hipSuccess && terms) e = hipMemcpyAsync(base + o_col, col + t0, terms * 4, hipMemcpyHostToDevice, S->compute);
    if (e == hipSuccess && terms) e = hipMemcpyAsync(base + o_cf, coeffs + (size_t)t0 * 4, terms * 32, hipMemcpyHostToDevice, S->compute);
    if (e == hipSuccess) e = hipStreamSynchronize(S->compute);   // (rp is a local vector)
    if (e != hipSuccess) return ZK_ERR_DEVICE;
    const int rc = sparse_matvec<F>(base + o_out, base + o_bases, n_bases, (const uint32_t*)(base + o_rp), (const uint32_t*)(base + o_col), base + o_cf, rows, terms,
                                    (void*)S->compute, group, g2_trusted, base + o_scr, scr_bytes);
    if (rc != ZK_OK) return rc;
    e = hipMemcpyAsync(out + r0 * rec, base + o_out, rows * rec, hipMemcpyDeviceToHost, S->compute);
    if (e == hipSuccess) e = hipStreamSynchronize(S->compute);
    return e == hipSuccess ? ZK_OK : ZK_ERR_DEVICE;
  };
  return first_error(fan_out(parts, run_range));
}

template int batch_exp_host<Fq>(uint8_t*, const uint8_t*, const uint64_t*, size_t, int, bool);
template int batch_exp_host<Fq2>(uint8_t*, const uint8_t*, const uint64_t*, size_t, int, bool);
template int dense_host<1>(const uint8_t*, const uint8_t*, const uint64_t*, size_t, uint64_t*, uint64_t*, const FrRandomStream*);
template int dense_host<2>(const uint8_t*, const uint8_t*, const uint64_t*, size_t, uint64_t*, uint64_t*, const FrRandomStream*);
template int sparse_matvec<Fq>(void*, const void*, size_t, const uint32_t*, const uint32_t*, const void*, size_t, size_t, void*, int, bool, void*, size_t);
template int sparse_matvec<Fq2>(void*, const void*, size_t, const uint32_t*, const uint32_t*, const void*, size_t, size_t, void*, int, bool, void*, size_t);
template int sparse_matvec_host<Fq>(uint8_t*, const uint8_t*, size_t, const uint32_t*, const uint32_t*, const uint64_t*, size_t, size_t, int, bool);
template int sparse_matvec_host<Fq2>(uint8_t*, const uint8_t*, size_t, const uint32_t*, const uint32_t*, const uint64_t*, size_t, size_t, int, bool);
}  // namespace zk
