// Radix-2 FFT over CURVE POINTS of BN254 (G1 and G2) for gfx950: EvaluationDomain<Point<G>>::{fft, ifft}; instantiated by
// point_fft.hip (G1) and point_fft_g2.hip (G2, its own translation unit: the Fq2 group law is the long compile).
//
// Reference path: bellman/src/group.rs:22-51 (`Point<G>`: group_mul_assign = scalar multiplication of a projective
// point by an Fr twiddle, add, sub) under bellman/src/domain.rs:154-173,274-317, driven by powersoftau/src/bin/prepare_phase2.rs:68-131
// (affine tau-powers -> ifft -> batch_normalization -> Lagrange-basis points) -- the dominant cost of `prepare_phase2`.
//
// Every butterfly is a 254-bit scalar multiplication, so the work is n/2 * log n * ~300k integer mads: pure ALU.
// Layout: a working array of U-form JACOBIAN points (curveu.hpp JacU / JacU2, every coordinate in the 2^261 domain, padded to whole
// 16-byte words: 112 B / 224 B) in HBM; one lane per butterfly per stage, DIT after a bit-reversed load.  The twiddle multiplication
// is the windowed program of window_mul.hpp over a per-lane table in a scratch array laid out [entry][lane]; the closing
// u + t / u - t run through the same loop, hence the same single inlined doubling and addition.
//   G1: the twiddle is split by the GLV endomorphism, 33 windows (exact on every point of the curve).
//   G2, default: 64 plain windows of the canonical twiddle -- the group law only, so the transform is the reference's (group.rs:38-51
//       over wnaf.rs:4-71) for EVERY vector of points of the twist.  MI355ZK_G2_TRUSTED_SUBGROUP: 33 windows split over psi, which is
//       mu in the order-r subgroup only; a transform of subgroup points stays in it.
// Input and output are affine raw records (64 B / 128 B, all-zero = infinity); the output is normalised with one inversion per 16 / 8
// points (scalar_mul.hip batch_normalize_*), i.e. it is what `batch_normalization` + `into_affine` leave (ec.rs:251-299, 596-629),
// which makes parity bit-exact.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdlib>

#include "../../include/mi355zk.h"
#include "device_mem.hpp"
#include "window_mul.hpp"

namespace zk {
namespace {

template <class G>
struct alignas(16) WorkPt {   // a working-array point
  typename G::Acc p;
  uint32_t pad[(16 - sizeof(typename G::Acc) % 16) / 4];
};
template <class G>
__device__ __forceinline__ void work_store(WorkPt<G>* at, const typename G::Acc& q) {
  WorkPt<G> r;
  r.p = q;
#pragma unroll
  for (uint32_t& w : r.pad) w = 0;
  copy16_store(at, r);
}

// affine raw records -> working points at the bit-reversed position (domain.rs:288-293)
template <class G>
__global__ void __launch_bounds__(256) pfft_load_kernel(const typename G::Aff* __restrict__ in, WorkPt<G>* __restrict__ work, uint32_t log_n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (1u << log_n)) return;
  const typename G::Aff a = in[i];
  uint32_t r = log_n ? (__brev(i) >> (32 - log_n)) : 0;
  work_store(work + r, a.is_zero() ? G::Acc::zero() : G::from_affine(a));
}

// mode 0: the butterfly of stage s, a[i0] = u + w t, a[i1] = u - w t (domain.rs:303-309): window_mul.hpp's program on t = a[i1], then
//   step STEP_STORE: entry 1 := product;  STEP_SUM / STEP_DIF: acc = u +/- entry 1, stored to a[i0] / a[i1]
// mode 1: every point times the scalar `c` (ifft's 1/m, domain.rs:163-173): the program alone.
template <class G, bool SPLIT>
__global__ void __launch_bounds__(256) pfft_stage_kernel(WorkPt<G>* __restrict__ work, const uint32_t* __restrict__ tw_canon, uint32_t log_n,
                                                        uint32_t s, uint64_t b0, uint64_t n_chunk, typename G::Tab* __restrict__ tab, int mode,
                                                        Fr c) {
  using Acc = typename G::Acc;
  using W = WindowMul<G, SPLIT, SPLIT ? 33 : 64>;   // twiddles are canonical
  const uint64_t t = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n_chunk) return;
  const uint64_t b = b0 + t;
  uint64_t i0, i1;
  uint32_t kk[8];
  bool unit = false;  // twiddle w^0 = 1
  if (mode == 0) {
    const uint64_t m = 1ull << s, j = b & (m - 1);
    i0 = ((b >> s) << (s + 1)) + j;
    i1 = i0 + m;
    unit = j == 0;
    const uint32_t* kp = tw_canon + (j << (log_n - 1 - s)) * 8;
#pragma unroll
    for (int l = 0; l < 8; ++l) kk[l] = kp[l];
  } else {
    i0 = i1 = b;
#pragma unroll
    for (int l = 0; l < 8; ++l) kk[l] = c.l[l];
  }
  const Acc u = mode == 0 ? copy16_load(work + i0).p : Acc::zero();
  Acc acc = copy16_load(work + i1).p;
  typename W::Mag mag1, mag2;
  typename W::Sgn sgn1, sgn2;
  bool neg1, neg2;
  typename G::Endo endo;
  W::digits(kk, mag1, sgn1, mag2, sgn2, neg1, neg2, endo);
  const bool t_inf = acc.is_zero();
  if (t_inf && mode == 1) return;   // c * infinity = infinity: the record stays
  tab += t;
  // Infinite operands take ONE path: an infinite point makes a table entry with Z == 0, and the executor skips such an entry --
  // adding infinity leaves the other operand, which is the group law's answer.
  copy16_store(tab, G::tab_entry(acc));   // entry 1 = 1t
  constexpr int STEP_STORE = W::STEPS, STEP_SUM = STEP_STORE + 1, STEP_DIF = STEP_STORE + 2;
  // t infinite, or the twiddle one: the product is t itself and entry 1 already holds it -- the multiplication is skipped
  const int first = (unit || t_inf) ? STEP_SUM : 0;
  const int last = mode == 0 ? STEP_DIF : STEP_STORE - 1;
#pragma unroll 1
  for (int step = first; step <= last; ++step) {
    WinStep st;
    if (step < STEP_STORE) {
      st = W::decode(step, mag1, sgn1, mag2, sgn2, neg1, neg2);
    } else if (step == STEP_STORE) {
      st.store = 1;   // entry 1 := the product (infinite: Z == 0, so both outputs below are u)
    } else {
      acc = u;
      st.add = 1;     // u +/- entry 1 (skipped when it is infinite: u +/- infinity = u)
      st.negate = step == STEP_DIF;
    }
    acc = W::template exec<false>(acc, st, tab, n_chunk, endo);
    if (step == STEP_SUM) work_store(work + i0, acc);
    if (step == STEP_DIF) work_store(work + i1, acc);
  }
  if (mode == 1) work_store(work + i0, acc);
}

// working points -> (X, Y) in the output record and Z in zbuf, memory format; the batched normalisation finishes
template <class G>
__global__ void __launch_bounds__(256) pfft_store_kernel(const WorkPt<G>* __restrict__ work, typename G::Aff* __restrict__ out,
                                                        typename G::Z* __restrict__ zbuf, uint32_t log_n) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= (1u << log_n)) return;
  const Jacobian<typename G::Z> r = G::to_std(copy16_load(work + i).p);
  out[i] = typename G::Aff{r.x, r.y};
  zbuf[i] = r.z;
}

// tw[e] = canonical(omega^e), e < count
__global__ void pfft_twiddle_kernel(uint32_t* tw, Fr omega, uint64_t count) {
  uint64_t e = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= count) return;
  Fr c = to_canonical(pow_u64(omega, e));
#pragma unroll
  for (int l = 0; l < 8; ++l) tw[e * 8 + l] = c.l[l];
}

// lanes per launch of a stage: the built-in limit, or (test hook, read on every call) MI355ZK_PFFT_CHUNK_TEST = a decimal count >= 1 below it, of ANY
// value -- the launch loop, a second launch over the same table and a ragged last launch then run at sizes the CPU oracle checks record by record
uint64_t pfft_lanes_per_launch(uint64_t built_in) {
  const char* env_test = std::getenv("MI355ZK_PFFT_CHUNK_TEST");
  const uint64_t v = env_test ? (uint64_t)std::strtoull(env_test, nullptr, 10) : 0;
  return v >= 1 && v < built_in ? v : built_in;
}

// d_points: 2^log_n affine raw records, in place.  scale: every output is multiplied by scale_canon (ifft: m^-1).  split: the twiddles go
// over the endomorphism (always, where it is exact everywhere).  normalize: io[i] = (X, Y), z[i] = Z -> affine records.
template <class G>
int point_fft(void* d_points, uint32_t log_n, const Fr& omega, bool scale, const Fr& scale_canon, hipStream_t st, bool split,
              int (*normalize)(void*, const void*, uint64_t, hipStream_t)) {
  using Tab = typename G::Tab;
  const uint64_t n = 1ull << log_n;
  const uint64_t lanes_max = scale ? n : (n >= 2 ? n / 2 : 1);
  const uint64_t limit = pfft_lanes_per_launch(G::PFFT_LANES);
  const uint64_t chunk = lanes_max < limit ? lanes_max : limit;  // table: 8 entries per lane
  const size_t o_work = 0, o_tw = o_work + ((n * sizeof(WorkPt<G>) + 255) & ~(size_t)255), o_z = o_tw + (((n / 2 + 1) * 32 + 255) & ~(size_t)255),
               o_tab = o_z + ((n * sizeof(typename G::Z) + 255) & ~(size_t)255), total = o_tab + 8 * chunk * sizeof(Tab);
  DevTemp buf;
  if (int rc = buf.alloc(total)) return rc;
  WorkPt<G>* work = buf.as<WorkPt<G>>(o_work);
  uint32_t* tw = buf.as<uint32_t>(o_tw);
  typename G::Z* zbuf = buf.as<typename G::Z>(o_z);
  Tab* tab = buf.as<Tab>(o_tab);
  auto stage = [&](uint32_t s, uint64_t b0, uint64_t m, int mode, const Fr& c) {
    const dim3 grid((unsigned)((m + 255) / 256)), block(256);
    if (G::ENDO_EVERYWHERE || split) hipLaunchKernelGGL((pfft_stage_kernel<G, true>), grid, block, 0, st, work, tw, log_n, s, b0, m, tab, mode, c);
    else hipLaunchKernelGGL((pfft_stage_kernel<G, G::ENDO_EVERYWHERE>), grid, block, 0, st, work, tw, log_n, s, b0, m, tab, mode, c);
  };
  if (n >= 2) hipLaunchKernelGGL(pfft_twiddle_kernel, dim3((unsigned)((n / 2 + 255) / 256)), dim3(256), 0, st, tw, omega, n / 2);
  hipLaunchKernelGGL(pfft_load_kernel<G>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, (const typename G::Aff*)d_points, work, log_n);
  for (uint32_t s = 0; s < log_n; ++s)
    for (uint64_t b0 = 0; b0 < n / 2; b0 += chunk) stage(s, b0, n / 2 - b0 < chunk ? n / 2 - b0 : chunk, 0, Fr::zero());
  if (scale)
    for (uint64_t b0 = 0; b0 < n; b0 += chunk) stage(0u, b0, n - b0 < chunk ? n - b0 : chunk, 1, scale_canon);
  hipLaunchKernelGGL(pfft_store_kernel<G>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, work, (typename G::Aff*)d_points, zbuf, log_n);
  ZK_HIP(hipGetLastError());
  const int rc = normalize(d_points, zbuf, n, st);
  ZK_HIP(hipStreamSynchronize(st));  // every stage and the normalisation are done with buf: it dies with this call
  return rc;
}

}  // namespace
}  // namespace zk
