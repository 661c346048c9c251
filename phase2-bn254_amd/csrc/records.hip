// Base vectors in the caller's record layout: the argument rules of the strided entry points (include/mi355zk.h) and the repack
// kernel that turns raw records -- bellman's `G1Affine { x: Fq, y: Fq, infinity: bool }` (72 B) / `G2Affine` (136 B), or any layout of
// the same fields -- into the packed records every MSM kernel reads (64 B x || y / 128 B x.c0 || x.c1 || y.c0 || y.c1; all-zero =
// infinity).  The host path (host_entry.hip: msm_host_run) uploads raw pieces and runs this kernel on its copy stream, so that the
// accumulate / partition / reduce / table kernels never see the caller's layout.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/mi355zk.h"
#include "api_internal.hpp"

namespace zk {

int records_layout_check(int group, size_t stride, size_t x_off, size_t y_off, size_t inf_off, RecordLayout* out) {
  if (group != 1 && group != 2) return ZK_ERR_BAD_ARGS;
  const size_t csz = group == 1 ? 32 : 64;  // bytes of one coordinate (Fq / Fq2)
  if (stride == 0 || stride % 4 || stride > 4096) return ZK_ERR_BAD_ARGS;
  if (x_off % 4 || y_off % 4) return ZK_ERR_BAD_ARGS;
  if (stride < csz || x_off > stride - csz || y_off > stride - csz) return ZK_ERR_BAD_ARGS;  // a coordinate runs past the record
  if (x_off < y_off + csz && y_off < x_off + csz) return ZK_ERR_BAD_ARGS;                     // x and y overlap
  if (inf_off != MI355ZK_NO_FLAG) {
    if (inf_off >= stride) return ZK_ERR_BAD_ARGS;
    if ((inf_off >= x_off && inf_off < x_off + csz) || (inf_off >= y_off && inf_off < y_off + csz)) return ZK_ERR_BAD_ARGS;
  }
  RecordLayout L;
  if (!(stride == 2 * csz && x_off == 0 && y_off == csz && inf_off == MI355ZK_NO_FLAG)) {  // else: the packed layout, today's path
    L.stride = stride;
    L.x_off = x_off;
    L.y_off = y_off;
    L.inf_off = inf_off;
  }
  if (out) *out = L;
  return ZK_OK;
}

// One lane per 16-byte piece of the packed output (PIECES = 4 per G1 record, 8 per G2 record): adjacent lanes store adjacent 16 B, so a
// wave writes 1 KiB contiguously (dwordx4 stores).  A lane's 16 B lie inside one coordinate of one raw record, read as one dwordx4
// (WIDE: stride, x_off, y_off and the buffer are 16-byte aligned) or four dwords.  Every lane of a record reads the record's flag byte
// (the same address: one cache line) and stores zeros when it is set.  Memory-bound; a grid-stride loop so that any n fits the grid.
template <int PIECES, bool WIDE>
__global__ __launch_bounds__(256) void records_pack(const uint8_t* __restrict__ raw, uint64_t n, uint32_t stride, uint32_t x_off,
                                                    uint32_t y_off, uint32_t inf_off, uint32_t has_flag, uint4* __restrict__ out) {
  constexpr uint32_t HALF = PIECES / 2;
  const uint64_t total = n * PIECES;
  for (uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += (uint64_t)gridDim.x * blockDim.x) {
    const uint64_t rec = t / PIECES;
    const uint32_t k = (uint32_t)(t % PIECES);
    const uint8_t* r = raw + rec * stride;
    const uint32_t off = (k < HALF ? x_off : y_off) + (k % HALF) * 16u;
    uint4 v = make_uint4(0u, 0u, 0u, 0u);
    if (!has_flag || r[inf_off] == 0) {
      if (WIDE) {
        v = *reinterpret_cast<const uint4*>(r + off);
      } else {
        const uint32_t* p = reinterpret_cast<const uint32_t*>(r + off);
        v = make_uint4(p[0], p[1], p[2], p[3]);
      }
    }
    out[t] = v;
  }
}

int records_pack_run(int group, const void* d_raw, size_t n, const RecordLayout& L, void* d_out, hipStream_t st) {
  if (n == 0) return ZK_OK;
  if (L.packed()) {  // (the packed layout: a plain copy)
    ZK_HIP(hipMemcpyAsync(d_out, d_raw, n * (group == 1 ? 64 : 128), hipMemcpyDeviceToDevice, st));
    return ZK_OK;
  }
  const bool wide = L.stride % 16 == 0 && L.x_off % 16 == 0 && L.y_off % 16 == 0 && (uintptr_t)d_raw % 16 == 0;
  const bool flag = L.inf_off != MI355ZK_NO_FLAG;
  const uint64_t total = (uint64_t)n * (group == 1 ? 4 : 8);
  const uint64_t want = (total + 255) / 256;
  const unsigned blocks = (unsigned)(want < (1u << 20) ? want : (1u << 20));
  const uint8_t* raw = (const uint8_t*)d_raw;
  const uint32_t s = (uint32_t)L.stride, x = (uint32_t)L.x_off, y = (uint32_t)L.y_off, f = flag ? (uint32_t)L.inf_off : 0u;
  uint4* out = (uint4*)d_out;
  if (group == 1) {
    if (wide) hipLaunchKernelGGL((records_pack<4, true>), dim3(blocks), dim3(256), 0, st, raw, (uint64_t)n, s, x, y, f, (uint32_t)flag, out);
    else hipLaunchKernelGGL((records_pack<4, false>), dim3(blocks), dim3(256), 0, st, raw, (uint64_t)n, s, x, y, f, (uint32_t)flag, out);
  } else {
    if (wide) hipLaunchKernelGGL((records_pack<8, true>), dim3(blocks), dim3(256), 0, st, raw, (uint64_t)n, s, x, y, f, (uint32_t)flag, out);
    else hipLaunchKernelGGL((records_pack<8, false>), dim3(blocks), dim3(256), 0, st, raw, (uint64_t)n, s, x, y, f, (uint32_t)flag, out);
  }
  ZK_HIP(hipGetLastError());
  return ZK_OK;
}

}  // namespace zk
