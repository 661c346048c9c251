// The random exponents rho of merge_pairs / power_pairs, generated where they are used (include/mi355zk.h; the generator: chacha.hpp).  The
// reference draws them on the host (powersoftau/src/utils.rs:116-123, phase2/src/utils.rs:79-86); brought by the caller they are 32 B per point
// over the link next to 64 B per G1 point, and host generator time over 2^20 .. 2^28 elements.  Here one lane computes one ChaCha20 block -- two
// scalars, 64 B, four 16-byte stores -- and the MSM that follows reads them from device memory as it reads a caller's.
//   fr_random_fill                     the kernel's launcher (device pointer, the caller's stream)
//   mi355zk_bn254_fr_random_dev        the same as an entry point
//   mi355zk_selftest_fr_random         the same scalars from a host loop over chacha.hpp (no device)
//   ..._merge_pairs_random_dev         rho into a stream-ordered workspace, then msm_g*_dense_device as merge_pairs_dev runs it
//   ..._merge_pairs_random             host buffers: dense_host with no exponent upload, each piece filling its own range of the stream
#include <hip/hip_runtime.h>

#include "../../include/mi355zk.h"
#include "chacha.hpp"

#include "api_internal.hpp"

namespace zk {
namespace {

constexpr unsigned FR_RANDOM_BLOCK = 256;

struct ChaChaKey {
  uint32_t w[8];
};

// Lane t computes block (first >> 1) + t and stores those of its two scalars that lie in [first, first + n): an odd `first` drops the
// low half of the first block, an odd first + n the high half of the last.  out is 16-byte aligned and holds n scalars of 32 B.
__global__ void __launch_bounds__(FR_RANDOM_BLOCK) fr_random_kernel(uint64_t* __restrict__ out, uint64_t n, ChaChaKey key, uint64_t stream_id,
                                                                    uint64_t first, uint64_t n_blocks) {
  const uint64_t t = (uint64_t)blockIdx.x * FR_RANDOM_BLOCK + threadIdx.x;
  if (t >= n_blocks) return;
  const uint64_t block = (first >> 1) + t;
  uint64_t lo[4], hi[4];
  fr_random_block(lo, hi, key.w, stream_id, block);
  const uint64_t g = 2 * block;   // (first + n <= 2^64 is the caller's: the index of a scalar is a u64)
  if (g >= first && g - first < n) {
    ulonglong2* dst = reinterpret_cast<ulonglong2*>(out + 4 * (g - first));
    dst[0] = make_ulonglong2(lo[0], lo[1]);
    dst[1] = make_ulonglong2(lo[2], lo[3]);
  }
  if (g + 1 - first < n) {   // g + 1 >= first always: block >= first >> 1
    ulonglong2* dst = reinterpret_cast<ulonglong2*>(out + 4 * (g + 1 - first));
    dst[0] = make_ulonglong2(hi[0], hi[1]);
    dst[1] = make_ulonglong2(hi[2], hi[3]);
  }
}

int fr_random_host(uint64_t* out, size_t n, const uint32_t key[8], uint64_t stream_id, uint64_t first) {
  if (!key || (n && !out) || n >= ((size_t)1 << 31)) return ZK_ERR_BAD_ARGS;
  for (size_t i = 0; i < n;) {
    const uint64_t g = first + i;
    uint64_t lo[4], hi[4];
    fr_random_block(lo, hi, key, stream_id, g >> 1);
    if ((g & 1) == 0) {
      for (int j = 0; j < 4; ++j) out[4 * i + j] = lo[j];
      ++i;
      if (i == n) break;
    }
    for (int j = 0; j < 4; ++j) out[4 * i + j] = hi[j];
    ++i;
  }
  return ZK_OK;
}

template <int GROUP>
int merge_pairs_random_dev(const void* d_v1, const void* d_v2, size_t n, const uint32_t key[8], uint64_t stream_id, void* stream, uint64_t* out_s,
                           uint64_t* out_sx) {
  if (!out_s || !out_sx || !key || (n && (!d_v1 || !d_v2)) || n >= ((size_t)1 << 31)) return ZK_ERR_BAD_ARGS;
  hipStream_t st = (hipStream_t)stream;
  void* d_rho = nullptr;
  if (n) {
    ZK_HIP(hipMallocAsync(&d_rho, n * 32, st));
    if (int rc = fr_random_fill(d_rho, n, key, stream_id, 0, st)) {
      (void)hipFreeAsync(d_rho, st);
      return rc;
    }
  }
  // (the sums come back to host memory: the stream is idle when this returns, and the workspace goes back in stream order behind it)
  int rc = GROUP == 1 ? msm_g1_dense_device(d_v1, d_v2, d_rho, n, st, out_s, out_sx) : msm_g2_dense_device(d_v1, d_v2, d_rho, n, st, out_s, out_sx);
  if (d_rho && hipFreeAsync(d_rho, st) != hipSuccess && rc == ZK_OK) rc = ZK_ERR_DEVICE;
  return rc;
}

template <int GROUP>
int merge_pairs_random_host(const uint8_t* v1, const uint8_t* v2, size_t n, const uint32_t key[8], uint64_t stream_id, uint64_t* out_s, uint64_t* out_sx) {
  if (!v2 || !key) return ZK_ERR_BAD_ARGS;
  FrRandomStream rnd;
  for (int i = 0; i < 8; ++i) rnd.key[i] = key[i];
  rnd.stream_id = stream_id;
  return dense_host<GROUP>(v1, v2, nullptr, n, out_s, out_sx, &rnd);
}

}  // namespace

int fr_random_fill(void* d_out, size_t n, const uint32_t key[8], uint64_t stream_id, uint64_t first, hipStream_t st) {
  if (n == 0) return ZK_OK;
  if (!d_out || !key || n >= ((size_t)1 << 31) || ((uintptr_t)d_out & 15) != 0 || first + n < first) return ZK_ERR_BAD_ARGS;
  static const int slot = prof_slot("fr_random");
  ChaChaKey k;
  for (int i = 0; i < 8; ++i) k.w[i] = key[i];
  const uint64_t n_blocks = ((first + n - 1) >> 1) - (first >> 1) + 1;   // <= 2^30 + 1
  prof_begin(slot, st);
  hipLaunchKernelGGL(fr_random_kernel, dim3((unsigned)((n_blocks + FR_RANDOM_BLOCK - 1) / FR_RANDOM_BLOCK)), dim3(FR_RANDOM_BLOCK), 0, st,
                     (uint64_t*)d_out, (uint64_t)n, k, stream_id, first, n_blocks);
  prof_end(slot, st);
  ZK_HIP(hipGetLastError());
  return ZK_OK;
}

}  // namespace zk

extern "C" {

int mi355zk_bn254_fr_random_dev(void* d_out, size_t n, const uint32_t key[8], uint64_t stream_id, uint64_t first, void* stream) {
  return zk::abi_guard([&]() -> int {
    if (!d_out || !key) return ZK_ERR_BAD_ARGS;  // (NULL is refused for n == 0 too: the rule of the header)
    return zk::fr_random_fill(d_out, n, key, stream_id, first, (hipStream_t)stream);
  });
}
int mi355zk_selftest_fr_random(uint64_t* out, size_t n, const uint32_t key[8], uint64_t stream_id, uint64_t first) {
  return zk::abi_guard([&]() -> int { return zk::fr_random_host(out, n, key, stream_id, first); });
}
int mi355zk_bn254_g1_merge_pairs_random_dev(const void* d_v1, const void* d_v2, size_t n, const uint32_t key[8], uint64_t stream_id, void* stream,
                                            uint64_t out_s[12], uint64_t out_sx[12]) {
  return zk::abi_guard([&]() -> int { return zk::merge_pairs_random_dev<1>(d_v1, d_v2, n, key, stream_id, stream, out_s, out_sx); });
}
int mi355zk_bn254_g2_merge_pairs_random_dev(const void* d_v1, const void* d_v2, size_t n, const uint32_t key[8], uint64_t stream_id, void* stream,
                                            uint64_t out_s[24], uint64_t out_sx[24]) {
  return zk::abi_guard([&]() -> int { return zk::merge_pairs_random_dev<2>(d_v1, d_v2, n, key, stream_id, stream, out_s, out_sx); });
}
int mi355zk_bn254_g1_merge_pairs_random(const uint8_t* v1, const uint8_t* v2, size_t n, const uint32_t key[8], uint64_t stream_id, uint64_t out_s[12],
                                        uint64_t out_sx[12]) {
  return zk::abi_guard([&]() -> int { return zk::merge_pairs_random_host<1>(v1, v2, n, key, stream_id, out_s, out_sx); });
}
int mi355zk_bn254_g2_merge_pairs_random(const uint8_t* v1, const uint8_t* v2, size_t n, const uint32_t key[8], uint64_t stream_id, uint64_t out_s[24],
                                        uint64_t out_sx[24]) {
  return zk::abi_guard([&]() -> int { return zk::merge_pairs_random_host<2>(v1, v2, n, key, stream_id, out_s, out_sx); });
}

}  // extern "C"
