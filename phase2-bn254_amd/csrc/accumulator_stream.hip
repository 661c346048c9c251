// Powers-of-tau accumulator files streamed through the device (include/mi355zk.h: mi355zk_bn254_g{1,2}_accumulator_transform and
// _accumulator_power_pairs).  The reference's only accumulator is BatchedAccumulator over mmap'ed files (powersoftau/src/batched_accumulator.rs):
// every binary takes a batch_size because a power-28 challenge is ~103 GB.  Here a call takes one chunk of one vector as WIRE records in host
// memory (an mmap'ed file range) and works it off in pieces of `piece` records:
//
//   copy stream      upload i+1 |                          download i-1 | upload i+2 ...
//   compute stream   piece i:  decode -> infinity scan (+ G2 membership) -> [fr_powers -> into_repr -> batch_exp -> scan -> encode]
//
// with two buffer sets, so that device memory is a fixed multiple of `piece` (the formula is in the header) and never a function of n.  The
// kernels are the library's own (codec.hip, field_ops.hip, scalar_mul.hip, fr_random.hip, the dense multiexp); the only kernel of this unit is
// the scan for the lowest all-zero record.  One host thread drives a call, as in batch_exp_host: the kernels of piece i + 1 are queued
// before the thread waits for piece i's download.  Several calls (one per vector, say) may run from several host threads: each leases its own
// stage and buffer.
#include <hip/hip_runtime.h>

#include <cstring>
#include <type_traits>

#include "../../include/mi355zk.h"
#include "curveu.hpp"
#include "device_util.hpp"
#include "api_internal.hpp"
#include "host_pools.hpp"

namespace zk {
namespace {

constexpr size_t DEFAULT_PIECE = (size_t)1 << 18;
constexpr unsigned long long NONE = ~0ull;
// the four words a piece reports through (set to NONE before its kernels): the decoder's minimum of (index << 8 | code), then the lowest index
// of an all-zero input record, of a G2 record outside the subgroup, of an all-zero output record
enum { W_DECODE = 0, W_INFINITY, W_SUBGROUP, W_OUT_INFINITY, W_COUNT };

// One lane per raw affine record (QUADS x 16 B): the lowest index of an all-zero record -> *lowest; with `member` (one byte per record, from
// g2_subgroup_flags) the lowest index of a record whose byte is 0 -> *lowest_out.
template <int QUADS>
__global__ void __launch_bounds__(256) infinity_scan_kernel(const uint4* __restrict__ recs, uint64_t n, const uint8_t* __restrict__ member,
                                                           unsigned long long* __restrict__ lowest, unsigned long long* __restrict__ lowest_out) {
  const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  uint32_t acc = 0;
#pragma unroll
  for (int k = 0; k < QUADS; ++k) {
    const uint4 v = recs[i * QUADS + k];
    acc |= v.x | v.y | v.z | v.w;
  }
  if (acc == 0) atomicMin(lowest, (unsigned long long)i);
  if (member != nullptr && member[i] == 0) atomicMin(lowest_out, (unsigned long long)i);
}

template <int GROUP>
int scan(const void* d_recs, size_t n, const uint8_t* d_member, unsigned long long* d_lowest, unsigned long long* d_lowest_out, hipStream_t st) {
  if (n == 0) return ZK_OK;
  hipLaunchKernelGGL((infinity_scan_kernel<GROUP * 4>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const uint4*)d_recs, (uint64_t)n, d_member,
                     d_lowest, d_lowest_out);
  ZK_HIP(hipGetLastError());
  return ZK_OK;
}

bool fr_canonical(const Fr& c) {
  for (int i = 7; i >= 0; --i)
    if (c.l[i] != FrParams::P[i]) return c.l[i] < FrParams::P[i];
  return false;
}

size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

int hip_fail(const char* what, hipError_t e) {
  std::fprintf(stderr, "[mi355zk] %s: HIP error %d (%s)\n", what, (int)e, hipGetErrorString(e));
  return ZK_ERR_DEVICE;
}

// what a piece's four words say, in the order the in-memory flow meets them (decoding, the point at infinity, membership); `base`: the
// call-relative index of the piece's first record
int piece_verdict(const unsigned long long w[W_COUNT], uint64_t base, long long* err_index) {
  int rc = ZK_OK;
  unsigned long long idx = 0;
  if (w[W_DECODE] != NONE) { rc = (int)(w[W_DECODE] & 0xff); idx = w[W_DECODE] >> 8; }
  else if (w[W_INFINITY] != NONE) { rc = ZK_ERR_POINT_AT_INFINITY; idx = w[W_INFINITY]; }
  else if (w[W_SUBGROUP] != NONE) { rc = ZK_ERR_NOT_IN_SUBGROUP; idx = w[W_SUBGROUP]; }
  else if (w[W_OUT_INFINITY] != NONE) { rc = ZK_ERR_POINT_AT_INFINITY; idx = w[W_OUT_INFINITY]; }
  if (rc != ZK_OK && err_index) *err_index = (long long)(base + idx);
  return rc;
}

}  // namespace

template <int GROUP>
int accumulator_transform(uint8_t* out, const uint8_t* in, size_t n, uint64_t first, const uint64_t* tau, const uint64_t* coeff, int in_compressed,
                          int out_compressed, int checked, uint32_t mode, size_t piece, long long* err_index) {
  using F = typename std::conditional<GROUP == 1, Fq, Fq2>::type;
  constexpr size_t rec = sizeof(Affine<F>);
  static_assert(rec == (GROUP == 1 ? 64 : 128), "raw record");
  if (err_index) *err_index = -1;
  if (!out || !in || !tau || n >= ((size_t)1 << 31) || piece == 1 || (mode & ~(uint32_t)MI355ZK_G2_TRUSTED_SUBGROUP) || first + n < first) return ZK_ERR_BAD_ARGS;
  Fr tau_c, coeff_c;
  std::memcpy(&tau_c, tau, 32);
  if (coeff) std::memcpy(&coeff_c, coeff, 32);
  if (!fr_canonical(tau_c) || (coeff && !fr_canonical(coeff_c))) return ZK_ERR_BAD_ARGS;
  if (n == 0) return ZK_OK;
  const Fr tau_m = from_canonical(tau_c), coeff_m = coeff ? from_canonical(coeff_c) : Fr::one();
  const bool g2_trusted = GROUP == 2 && (mode & MI355ZK_G2_TRUSTED_SUBGROUP) != 0;
  const size_t in_rec = in_compressed ? rec / 2 : rec, out_rec = out_compressed ? rec / 2 : rec;
  if (piece == 0) piece = DEFAULT_PIECE;
  const size_t m_max = n < piece ? n : piece;
  // one buffer set: wire in, decoded points, exponents, products, wire out, the four words
  const size_t o_pts = al256(m_max * in_rec), o_sc = o_pts + al256(m_max * rec), o_res = o_sc + al256(m_max * 32), o_enc = o_res + al256(m_max * rec),
               o_err = o_enc + al256(m_max * out_rec), set_bytes = o_err + 256;
  int dev = 0;
  ZK_HIP(hipGetDevice(&dev));
  Events ev(4);   // (declared before the lease: destroyed after both streams are idle)
  hipEvent_t* up = &ev.e[0];
  hipEvent_t* done = &ev.e[2];
  CallLease lease;
  int rc = lease.open(dev, 2 * set_bytes);
  if (rc) return rc;
  HostStage* S = lease.S;
  char* set[2] = {(char*)lease.buf, (char*)lease.buf + set_bytes};
  hipError_t e = ev.create();
  if (e != hipSuccess) return hip_fail("accumulator_transform", e);
  const size_t n_pieces = (n + piece - 1) / piece;
  auto upload_and_launch = [&](size_t i) -> bool {   // false: rc, or else e, says why
    const size_t p0 = i * piece, m = n - p0 < piece ? n - p0 : piece;
    const int k = (int)(i & 1);
    char* b = set[k];
    unsigned long long* w = (unsigned long long*)(b + o_err);
    if ((e = hipMemcpyAsync(b, in + p0 * in_rec, m * in_rec, hipMemcpyHostToDevice, S->copy)) != hipSuccess) return false;
    if ((e = hipEventRecord(up[k], S->copy)) != hipSuccess || (e = hipStreamWaitEvent(S->compute, up[k], 0)) != hipSuccess) return false;
    if ((e = hipMemsetAsync(w, 0xff, W_COUNT * 8, S->compute)) != hipSuccess) return false;
    if ((rc = codec_decode_enqueue(GROUP, b + o_pts, b, m, in_compressed, checked, S->compute, w + W_DECODE))) return false;
    if ((rc = scan<GROUP>(b + o_pts, m, nullptr, w + W_INFINITY, nullptr, S->compute))) return false;
    // coeff * tau^(first + p0 + j), j < m: Montgomery from fr_powers, canonical for batch_exp
    const Fr c0 = mul(coeff_m, pow_u64(tau_m, first + p0));
    if ((rc = fr_powers((Fr*)(b + o_sc), tau_m, c0, m, S->compute))) return false;
    if ((rc = fr_into_repr((Fr*)(b + o_sc), (const Fr*)(b + o_sc), m, S->compute))) return false;
    if ((rc = batch_exp<F>(b + o_res, b + o_pts, 0, b + o_sc, 0, m, (void*)S->compute, nullptr, false, g2_trusted))) return false;
    if ((rc = scan<GROUP>(b + o_res, m, nullptr, w + W_OUT_INFINITY, nullptr, S->compute))) return false;
    if ((rc = codec_encode(GROUP, b + o_enc, b + o_res, m, out_compressed, S->compute))) return false;
    return (e = hipEventRecord(done[k], S->compute)) == hipSuccess;
  };
  for (size_t i = 0; i < 2 && i < n_pieces; ++i)
    if (!upload_and_launch(i)) return rc ? rc : hip_fail("accumulator_transform", e);
  for (size_t i = 0; i < n_pieces; ++i) {
    const size_t p0 = i * piece, m = n - p0 < piece ? n - p0 : piece;
    const int k = (int)(i & 1);
    unsigned long long w[W_COUNT];
    if ((e = hipStreamWaitEvent(S->copy, done[k], 0)) != hipSuccess) return hip_fail("accumulator_transform", e);
    if ((e = hipMemcpyAsync(out + p0 * out_rec, set[k] + o_enc, m * out_rec, hipMemcpyDeviceToHost, S->copy)) != hipSuccess) return hip_fail("accumulator_transform", e);
    if ((e = hipMemcpyAsync(w, set[k] + o_err, sizeof w, hipMemcpyDeviceToHost, S->copy)) != hipSuccess) return hip_fail("accumulator_transform", e);
    if ((e = hipStreamSynchronize(S->copy)) != hipSuccess) return hip_fail("accumulator_transform", e);   // piece i is on the host; its buffers are free
    if ((rc = piece_verdict(w, p0, err_index))) return rc;   // (the lease waits for what is still queued)
    if (i + 2 < n_pieces && !upload_and_launch(i + 2)) return rc ? rc : hip_fail("accumulator_transform", e);
  }
  if ((e = hipStreamSynchronize(S->compute)) != hipSuccess) return hip_fail("accumulator_transform", e);
  return ZK_OK;
}

template <int GROUP>
int accumulator_power_pairs(const uint8_t* in, size_t n, int compressed, int checked, int check_subgroup, const uint32_t* key, uint64_t stream_id,
                            uint64_t first, uint8_t* out_uncompressed, size_t piece, uint64_t* out_s, uint64_t* out_sx, long long* err_index) {
  using J = typename std::conditional<GROUP == 1, G1Jacobian, G2Jacobian>::type;
  constexpr size_t rec = GROUP == 1 ? 64 : 128;
  if (err_index) *err_index = -1;
  if (!in || !key || !out_s || !out_sx || n >= ((size_t)1 << 31) || piece == 1 || first + n < first) return ZK_ERR_BAD_ARGS;
  J total = J::zero(), total2 = J::zero();
  if (n > 0) {
    const bool membership = GROUP == 2 && check_subgroup != 0;
    const size_t in_rec = compressed ? rec / 2 : rec;
    if (piece == 0) piece = DEFAULT_PIECE;
    const size_t m_max = n < piece ? n : piece;   // records per piece: a piece of c records holds c - 1 terms and shares its last record with the next
    // one buffer set: wire in, decoded points, wire out (uncompressed), membership bytes, the four words; the exponents are shared (the dense
    // multiexp has returned before the next piece fills them)
    const size_t o_pts = al256(m_max * in_rec), o_enc = o_pts + al256(m_max * rec), o_mem = o_enc + (out_uncompressed ? al256(m_max * rec) : 0),
                 o_err = o_mem + (membership ? al256(m_max) : 0), set_bytes = o_err + 256;
    int dev = 0;
    ZK_HIP(hipGetDevice(&dev));
    Events ev(4);   // (declared before the lease: destroyed after both streams are idle)
    hipEvent_t* up = &ev.e[0];
    hipEvent_t* done = &ev.e[2];
    CallLease lease;
    int rc = lease.open(dev, 2 * set_bytes + al256(m_max * 32));
    if (rc) return rc;
    HostStage* S = lease.S;
    char* set[2] = {(char*)lease.buf, (char*)lease.buf + set_bytes};
    char* d_rho = (char*)lease.buf + 2 * set_bytes;
    hipError_t e = ev.create();
    if (e != hipSuccess) return hip_fail("accumulator_power_pairs", e);
    auto upload = [&](size_t r0, size_t cnt, int k) -> bool {
      if ((e = hipMemcpyAsync(set[k], in + r0 * in_rec, cnt * in_rec, hipMemcpyHostToDevice, S->copy)) != hipSuccess) return false;
      return (e = hipEventRecord(up[k], S->copy)) == hipSuccess;
    };
    size_t r0 = 0, cnt = m_max;
    if (!upload(r0, cnt, 0)) return hip_fail("accumulator_power_pairs", e);
    for (int k = 0;; k ^= 1) {
      const bool last = r0 + cnt == n;
      const size_t next_r0 = r0 + cnt - 1, next_cnt = last ? 0 : (n - next_r0 < piece ? n - next_r0 : piece);
      char* b = set[k];
      unsigned long long* w = (unsigned long long*)(b + o_err);
      uint8_t* d_member = membership ? (uint8_t*)(b + o_mem) : nullptr;
      // ---- piece (r0, cnt) on the compute stream, up to the re-encoded records
      if ((e = hipStreamWaitEvent(S->compute, up[k], 0)) != hipSuccess) return hip_fail("accumulator_power_pairs", e);
      if ((e = hipMemsetAsync(w, 0xff, W_COUNT * 8, S->compute)) != hipSuccess) return hip_fail("accumulator_power_pairs", e);
      if ((rc = codec_decode_enqueue(GROUP, b + o_pts, b, cnt, compressed, checked, S->compute, w + W_DECODE))) return rc;
      if (membership && (rc = g2_subgroup_flags(b + o_pts, cnt, (void*)S->compute, d_member))) return rc;
      if ((rc = scan<GROUP>(b + o_pts, cnt, d_member, w + W_INFINITY, w + W_SUBGROUP, S->compute))) return rc;
      if (out_uncompressed && (rc = codec_encode(GROUP, b + o_enc, b + o_pts, cnt, 0, S->compute))) return rc;
      if ((e = hipEventRecord(done[k], S->compute)) != hipSuccess) return hip_fail("accumulator_power_pairs", e);
      // ---- the next piece crosses the link meanwhile (its buffer set is free: the previous piece's download has returned)
      if (!last && !upload(next_r0, next_cnt, k ^ 1)) return hip_fail("accumulator_power_pairs", e);
      // ---- this piece's records and verdict come back
      unsigned long long hw[W_COUNT];
      if ((e = hipStreamWaitEvent(S->copy, done[k], 0)) != hipSuccess) return hip_fail("accumulator_power_pairs", e);
      if (out_uncompressed && (e = hipMemcpyAsync(out_uncompressed + r0 * rec, b + o_enc, cnt * rec, hipMemcpyDeviceToHost, S->copy)) != hipSuccess)
        return hip_fail("accumulator_power_pairs", e);
      if ((e = hipMemcpyAsync(hw, w, sizeof hw, hipMemcpyDeviceToHost, S->copy)) != hipSuccess) return hip_fail("accumulator_power_pairs", e);
      if ((e = hipStreamSynchronize(S->copy)) != hipSuccess) return hip_fail("accumulator_power_pairs", e);
      if ((rc = piece_verdict(hw, r0, err_index))) return rc;
      // ---- its cnt - 1 terms: rho_(first + r0 + j) * (v[r0 + j], v[r0 + j + 1]) -- one decoded array seen at two offsets
      if (cnt > 1) {
        const size_t m = cnt - 1;
        if ((rc = fr_random_fill(d_rho, m, key, stream_id, first + r0, S->compute))) return rc;
        J a = J::zero(), c = J::zero();
        rc = GROUP == 1 ? msm_g1_dense_device(b + o_pts, b + o_pts + rec, d_rho, m, S->compute, reinterpret_cast<uint64_t*>(&a), reinterpret_cast<uint64_t*>(&c))
                        : msm_g2_dense_device(b + o_pts, b + o_pts + rec, d_rho, m, S->compute, reinterpret_cast<uint64_t*>(&a), reinterpret_cast<uint64_t*>(&c));
        if (rc != ZK_OK) return rc;
        jac_add(total, a);
        jac_add(total2, c);
      }
      if (last) break;
      r0 = next_r0;
      cnt = next_cnt;
    }
  }
  std::memcpy(out_s, &total, sizeof total);
  std::memcpy(out_sx, &total2, sizeof total2);
  return ZK_OK;
}

// Wire records in host memory -> a vector of raw affine records that stays on the device (mi355zk_bn254_g{1,2}_points_load): the decoder
// writes each piece straight into the caller's vector, so a buffer set holds the piece's wire bytes, its membership bytes and the four words.
//
//   copy stream      upload i+1 |               words i | upload i+2 ...
//   compute stream   piece i:  decode -> (G2 membership) -> infinity scan
template <int GROUP>
int points_load(void* d_out, const uint8_t* in, size_t n, int compressed, int checked, int check_subgroup, size_t piece, long long* err_index) {
  constexpr size_t rec = GROUP == 1 ? 64 : 128;
  if (err_index) *err_index = -1;
  if (piece == 0) piece = DEFAULT_PIECE;
  if (piece >= ((size_t)1 << 31) || n > (~(size_t)0) / rec) return ZK_ERR_BAD_ARGS;
  if (n == 0) return ZK_OK;
  if (!d_out || !in || (uintptr_t)d_out % 16 != 0) return ZK_ERR_BAD_ARGS;
  const bool membership = GROUP == 2 && check_subgroup != 0;
  const size_t in_rec = compressed ? rec / 2 : rec;
  const size_t m_max = n < piece ? n : piece;
  const size_t o_mem = al256(m_max * in_rec), o_err = o_mem + (membership ? al256(m_max) : 0), set_bytes = o_err + 256;
  int dev = 0;
  ZK_HIP(hipGetDevice(&dev));
  Events ev(4);   // (declared before the lease: destroyed after both streams are idle)
  hipEvent_t* up = &ev.e[0];
  hipEvent_t* done = &ev.e[2];
  CallLease lease;
  int rc = lease.open(dev, 2 * set_bytes);
  if (rc) return rc;
  HostStage* S = lease.S;
  char* set[2] = {(char*)lease.buf, (char*)lease.buf + set_bytes};
  hipError_t e = ev.create();
  if (e != hipSuccess) return hip_fail("points_load", e);
  const size_t n_pieces = (n + piece - 1) / piece;
  auto upload_and_launch = [&](size_t i) -> bool {   // false: rc, or else e, says why
    const size_t p0 = i * piece, m = n - p0 < piece ? n - p0 : piece;
    const int k = (int)(i & 1);
    char* b = set[k];
    char* dst = (char*)d_out + p0 * rec;
    unsigned long long* w = (unsigned long long*)(b + o_err);
    uint8_t* d_member = membership ? (uint8_t*)(b + o_mem) : nullptr;
    if ((e = hipMemcpyAsync(b, in + p0 * in_rec, m * in_rec, hipMemcpyHostToDevice, S->copy)) != hipSuccess) return false;
    if ((e = hipEventRecord(up[k], S->copy)) != hipSuccess || (e = hipStreamWaitEvent(S->compute, up[k], 0)) != hipSuccess) return false;
    if ((e = hipMemsetAsync(w, 0xff, W_COUNT * 8, S->compute)) != hipSuccess) return false;
    if ((rc = codec_decode_enqueue(GROUP, dst, b, m, compressed, checked, S->compute, w + W_DECODE))) return false;
    if (membership && (rc = g2_subgroup_flags(dst, m, (void*)S->compute, d_member))) return false;
    if ((rc = scan<GROUP>(dst, m, d_member, w + W_INFINITY, w + W_SUBGROUP, S->compute))) return false;
    return (e = hipEventRecord(done[k], S->compute)) == hipSuccess;
  };
  for (size_t i = 0; i < 2 && i < n_pieces; ++i)
    if (!upload_and_launch(i)) return rc ? rc : hip_fail("points_load", e);
  for (size_t i = 0; i < n_pieces; ++i) {
    const int k = (int)(i & 1);
    unsigned long long w[W_COUNT];
    if ((e = hipStreamWaitEvent(S->copy, done[k], 0)) != hipSuccess) return hip_fail("points_load", e);
    if ((e = hipMemcpyAsync(w, set[k] + o_err, sizeof w, hipMemcpyDeviceToHost, S->copy)) != hipSuccess) return hip_fail("points_load", e);
    if ((e = hipStreamSynchronize(S->copy)) != hipSuccess) return hip_fail("points_load", e);   // piece i is decoded; its buffers are free
    if ((rc = piece_verdict(w, i * piece, err_index))) return rc;   // (the lease waits for what is still queued)
    if (i + 2 < n_pieces && !upload_and_launch(i + 2)) return rc ? rc : hip_fail("points_load", e);
  }
  if ((e = hipStreamSynchronize(S->compute)) != hipSuccess) return hip_fail("points_load", e);
  return ZK_OK;
}

// The inverse (mi355zk_bn254_g{1,2}_points_store): piece i + 1 is encoded while piece i crosses the link; a buffer set is the piece's wire bytes.
template <int GROUP>
int points_store(uint8_t* out, const void* d_in, size_t n, int compressed, size_t piece) {
  constexpr size_t rec = GROUP == 1 ? 64 : 128;
  if (piece == 0) piece = DEFAULT_PIECE;
  if (piece >= ((size_t)1 << 31) || n > (~(size_t)0) / rec) return ZK_ERR_BAD_ARGS;
  if (n == 0) return ZK_OK;
  if (!out || !d_in || (uintptr_t)d_in % 16 != 0) return ZK_ERR_BAD_ARGS;
  const size_t out_rec = compressed ? rec / 2 : rec;
  const size_t m_max = n < piece ? n : piece;
  const size_t set_bytes = al256(m_max * out_rec);
  int dev = 0;
  ZK_HIP(hipGetDevice(&dev));
  Events ev(2);   // (declared before the lease: destroyed after both streams are idle)
  hipEvent_t* done = &ev.e[0];
  CallLease lease;
  int rc = lease.open(dev, 2 * set_bytes);
  if (rc) return rc;
  HostStage* S = lease.S;
  char* set[2] = {(char*)lease.buf, (char*)lease.buf + set_bytes};
  hipError_t e = ev.create();
  if (e != hipSuccess) return hip_fail("points_store", e);
  const size_t n_pieces = (n + piece - 1) / piece;
  auto launch = [&](size_t i) -> bool {
    const size_t p0 = i * piece, m = n - p0 < piece ? n - p0 : piece;
    const int k = (int)(i & 1);
    if ((rc = codec_encode(GROUP, set[k], (const char*)d_in + p0 * rec, m, compressed, S->compute))) return false;
    return (e = hipEventRecord(done[k], S->compute)) == hipSuccess;
  };
  for (size_t i = 0; i < 2 && i < n_pieces; ++i)
    if (!launch(i)) return rc ? rc : hip_fail("points_store", e);
  for (size_t i = 0; i < n_pieces; ++i) {
    const size_t p0 = i * piece, m = n - p0 < piece ? n - p0 : piece;
    const int k = (int)(i & 1);
    if ((e = hipStreamWaitEvent(S->copy, done[k], 0)) != hipSuccess) return hip_fail("points_store", e);
    if ((e = hipMemcpyAsync(out + p0 * out_rec, set[k], m * out_rec, hipMemcpyDeviceToHost, S->copy)) != hipSuccess) return hip_fail("points_store", e);
    if ((e = hipStreamSynchronize(S->copy)) != hipSuccess) return hip_fail("points_store", e);   // piece i is on the host; its buffer is free
    if (i + 2 < n_pieces && !launch(i + 2)) return rc ? rc : hip_fail("points_store", e);
  }
  return ZK_OK;
}

template int points_load<1>(void*, const uint8_t*, size_t, int, int, int, size_t, long long*);
template int points_load<2>(void*, const uint8_t*, size_t, int, int, int, size_t, long long*);
template int points_store<1>(uint8_t*, const void*, size_t, int, size_t);
template int points_store<2>(uint8_t*, const void*, size_t, int, size_t);
template int accumulator_transform<1>(uint8_t*, const uint8_t*, size_t, uint64_t, const uint64_t*, const uint64_t*, int, int, int, uint32_t, size_t, long long*);
template int accumulator_transform<2>(uint8_t*, const uint8_t*, size_t, uint64_t, const uint64_t*, const uint64_t*, int, int, int, uint32_t, size_t, long long*);
template int accumulator_power_pairs<1>(const uint8_t*, size_t, int, int, int, const uint32_t*, uint64_t, uint64_t, uint8_t*, size_t, uint64_t*, uint64_t*, long long*);
template int accumulator_power_pairs<2>(const uint8_t*, size_t, int, int, int, const uint32_t*, uint64_t, uint64_t, uint8_t*, size_t, uint64_t*, uint64_t*, long long*);
}  // namespace zk
