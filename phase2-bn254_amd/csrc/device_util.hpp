// Shared host-side helpers for the HIP translation units of libmi355zk.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdio>

#include "host_util.hpp"  // return codes of the C ABI, JoinPool

#define ZK_HIP(expr)                                                                              \
  do {                                                                                            \
    hipError_t zk_e_ = (expr);                                                                    \
    if (zk_e_ != hipSuccess) {                                                                    \
      std::fprintf(stderr, "[mi355zk] HIP error %d (%s) at %s:%d: %s\n", (int)zk_e_,              \
                   hipGetErrorString(zk_e_), __FILE__, __LINE__, #expr);                          \
      return ZK_ERR_DEVICE;                                                                       \
    }                                                                                             \
  } while (0)

namespace zk {

// Copies of a record made of whole 16-byte words (alignas(16), sizeof a multiple of 16) between memory and registers: one
// dwordx4 access per word on the device, a plain copy on the host.
template <class T>
__host__ __device__ __forceinline__ T copy16_load(const T* p) {
  static_assert(alignof(T) % 16 == 0 && sizeof(T) % 16 == 0, "16-byte copies");
#if defined(__HIP_DEVICE_COMPILE__)
  T r;
  const uint4* q = reinterpret_cast<const uint4*>(p);
  uint4* d = reinterpret_cast<uint4*>(&r);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 16); ++i) d[i] = q[i];
  return r;
#else
  return *p;
#endif
}
template <class T>
__host__ __device__ __forceinline__ void copy16_store(T* p, const T& v) {
  static_assert(alignof(T) % 16 == 0 && sizeof(T) % 16 == 0, "16-byte copies");
#if defined(__HIP_DEVICE_COMPILE__)
  const uint4* s = reinterpret_cast<const uint4*>(&v);
  uint4* d = reinterpret_cast<uint4*>(p);
#pragma unroll
  for (int i = 0; i < (int)(sizeof(T) / 16); ++i) d[i] = s[i];
#else
  *p = v;
#endif
}

// A multiexp whose exponents arrive in CHUNKS: the host-buffer entry point (host_entry.hip: msm_host_entry) uploads them over PCIe while
// the kernels of the earlier chunks run.  msm_device (msm_host.hpp) evaluates chunk c = exponents [cuts[c], cuts[c+1]) when told
// where they are, with ONE geometry and ONE bucket array for the whole call.
struct MsmChunks {
  uint32_t n_chunks = 0;
  const uint64_t* cuts = nullptr;  // n_chunks + 1 exponent indices: 0 = cuts[0] < ... < cuts[n_chunks] = n, inner cuts multiples of 32
  // the device pointer of chunk c's exponents; makes `st` wait (device-side) until they have arrived
  virtual int acquire(uint32_t c, hipStream_t st, const void** d_scalars) = 0;
  // the digit kernel of chunk c -- the only reader of its exponents -- has been enqueued on `st`
  virtual int digits_enqueued(uint32_t c, hipStream_t st) = 0;
  virtual ~MsmChunks() {}
};

// Lightweight per-kernel timing used by bench.py's roofline leg: when enabled, the library brackets
// the named kernels with hipEvents on the launch stream and accumulates their durations.
struct KernelTimer {
  const char* name;
  double total_ms = 0.0;
  long count = 0;
};

void prof_enable(int on);   // 0 off, 1 every slot, 2 only the slot of prof_only
void prof_only(const char* name);
bool prof_enabled();
// record start/stop events around a launch on `st`; resolved lazily by prof_collect()
void prof_begin(int slot, hipStream_t st);
void prof_end(int slot, hipStream_t st);
void prof_collect();
int prof_slot(const char* name);  // find-or-create
bool prof_get(const char* name, double* total_ms, long* count);
void prof_reset();

// Every extern "C" entry point runs its body through one of these: the library's hosts are C / Rust / ctypes callers, and a C++
// exception (std::bad_alloc from a staging vector, std::system_error from a lock) must not unwind across that boundary.  It becomes
// a device error (rc < 0: the caller falls back to its own CPU path).
template <class Fn>
inline int abi_guard(Fn&& fn) noexcept {
  try {
    return fn();
  } catch (...) {
    return ZK_ERR_DEVICE;
  }
}
template <class Fn>
inline void abi_guard_void(Fn&& fn) noexcept {
  try {
    fn();
  } catch (...) {
  }
}

}  // namespace zk
