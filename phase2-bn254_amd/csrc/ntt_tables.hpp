#pragma once
// The NTT's device-resident state behind the planner (ntt_plan.hpp) and the launcher (ntt.hip: ntt_run_batch): the cache of power tables
// per (device, size, root) with their folded sets, and the per-stream inter-pass scratch.  Included by ntt.hip alone, below the kernels
// (the builders launch the table kernels and use UTab / TwU, which ntt.hip defines above the include).  Locking order: g_run_mu, then g_mu.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <utility>
#include <vector>

#include "device_mem.hpp"
#include "device_util.hpp"
#include "ntt_plan.hpp"

namespace zk {

namespace {

struct Key {
  int dev;
  uint32_t log_n;
  uint32_t w[8];
  bool operator<(const Key& o) const {
    if (dev != o.dev) return dev < o.dev;
    if (log_n != o.log_n) return log_n < o.log_n;
    for (int i = 0; i < 8; ++i)
      if (w[i] != o.w[i]) return w[i] < o.w[i];
    return false;
  }
};

// Per (device, log_n, omega) tables; built once and kept (the prover reuses one domain size for
// every fft of a proof: bellman/src/groth16/prover.rs:217-241).
// hipMalloc that adds to the owner's byte count (the table cache is bounded by BYTES per device: tables_make_room)
template <class T>
static hipError_t tab_malloc(T** p, size_t bytes, size_t* account) {
  hipError_t e = hipMalloc(p, bytes);
  if (e == hipSuccess) *account += bytes;
  return e;
}
struct PowTables {
  size_t bytes = 0;        // device bytes of A, B, roots, full (folded tables count in their own `bytes`)
  uint32_t h = 0;          // w^e = A[e >> h] * B[e & (2^h-1)], e < 2^log_n
  UTab* A = nullptr;
  UTab* B = nullptr;
  UTab* roots[NTT_MAX_LOG_NP + 1] = {};  // roots[b][x] = (w^(N/2^b))^x, x < 2^(b-1)
  UTab* full = nullptr;    // two-pass transforms up to NTT_FULL_TW_MAX_LOG: w^(k * col) at the first pass's output position (72 B per element)
  uint32_t full_log_s = 0;
  // (round 5) `full` with a transform's scale factors folded in (ntt_full_folded_kernel), one per (pre_g, post_c, post_g) this root has
  // been used with -- a domain uses two roots with two each: (fft, coset_fft) and (ifft, icoset_fft)
  struct Folded {
    size_t bytes = 0;
    bool has_pre = false, has_post_c = false, has_post_g = false;
    Fr pre{}, post_c{}, post_g{};
    uint32_t log_s = 0;
    UTab* full = nullptr;
    UTab* pre_rows = nullptr;   // (pre^S)^x, x < N_1
    UTab* pre_stages = nullptr; // the first pass's butterfly twiddles times the row twist (ntt_stage_table_kernel), N_1 entries
    UTab* post_rows = nullptr;  // (post^N_1)^k2, k2 < S  (in general: (post^(N / N_last))^k, k < N_last)
    // transforms without a full table (2^21 and up):
    bool big = false;
    UTab* pre_cols = nullptr;    // pre^col, col < N / N_first
    UTab* post_rowc = nullptr;   // post_c * post^rb, rb < N / N_last: the factor shared by the outputs of one row of the last pass
    UTab* tw_b_scaled = nullptr; // ifft: the low table B of the two-level twiddle times post_c -- the pass before the last multiplies it in
    void free_tabs() {
      (void)hipFree(full); (void)hipFree(pre_rows); (void)hipFree(pre_stages); (void)hipFree(post_rows);
      (void)hipFree(pre_cols); (void)hipFree(post_rowc); (void)hipFree(tw_b_scaled);
    }
  };
  std::vector<Folded> folded;
  void free_all() {
    (void)hipFree(A);
    (void)hipFree(B);
    (void)hipFree(full);
    for (auto* r : roots) (void)hipFree(r);
    for (auto& f : folded) f.free_tabs();
    folded.clear();
  }
};
constexpr size_t NTT_FOLDED_MAX = 4;   // per root: a caller cycling through coset generators must not grow device memory without limit

std::mutex g_mu;
std::map<Key, PowTables> g_tables;

// The cache is keyed on arbitrary roots (best_fft takes a caller-supplied omega): bounded per device, so that a caller cycling through
// roots cannot grow device memory without limit.  Called ONCE at the start of a transform (under g_run_mu), before any of its up to
// three table lookups: a drop between two lookups of one call would free the tables the first lookup has just returned (found by the
// NTT fuzz: 64 + entries in one process).  Dropping this device's entries is safe once the device is idle.
constexpr size_t NTT_TABLES_MAX = 64;
// ... and by BYTES: an entry is small up to 2^20 except for its full tables -- 72 B x 2^log_n each, up to 1 + NTT_FOLDED_MAX per
// root -- so 64 entries could hold ~18 GiB.  Default budget 4 GiB per device (env MI355ZK_NTT_TABLES_GB): a prover's two roots with their
// folded tables at 2^20 are 0.3 GiB.
static size_t tables_byte_budget() {
  const double gb = ntt_knobs().tables_gb;
  return (size_t)((gb > 0.03125 ? gb : 0.03125) * 1073741824.0);
}
int tables_make_room(size_t need) {
  int dev = 0;
  ZK_HIP(hipGetDevice(&dev));
  {
    std::lock_guard<std::mutex> lk(g_mu);
    size_t mine = 0, bytes = 0;
    for (auto& kv : g_tables) {
      if (kv.first.dev != dev) continue;
      ++mine;
      bytes += kv.second.bytes;
      for (auto& f : kv.second.folded) bytes += f.bytes;
    }
    if (mine + need <= NTT_TABLES_MAX && bytes <= tables_byte_budget()) return ZK_OK;
  }
  // the device drains OUTSIDE g_mu (callers on other devices keep looking their tables up); g_run_mu, held by the caller, keeps new
  // launches of THIS cache's tables from starting meanwhile
  ZK_HIP(hipDeviceSynchronize());
  std::lock_guard<std::mutex> lk(g_mu);
  for (auto it = g_tables.begin(); it != g_tables.end();) {
    if (it->first.dev != dev) { ++it; continue; }
    it->second.free_all();
    it = g_tables.erase(it);
  }
  return ZK_OK;
}

int build_pow_tables(hipStream_t st, uint32_t log_n, const Fr& w, bool want_roots, const uint32_t* bs, int nb, PowTables** out,
                     uint32_t full_log_s = 0) {
  int dev = 0;
  ZK_HIP(hipGetDevice(&dev));
  Key key;
  key.dev = dev;
  key.log_n = log_n;
  for (int i = 0; i < 8; ++i) key.w[i] = w.l[i];
  std::lock_guard<std::mutex> lk(g_mu);
  PowTables& T = g_tables[key];
  bool built = false;
  // on any failure the entry is removed again: a half-built entry (A set, B or a roots table missing) would be taken for
  // complete by the next call
  auto fail = [&](hipError_t e, const char* what) {
    std::fprintf(stderr, "[mi355zk] NTT table build failed (%s): %s\n", what, hipGetErrorString(e));
    (void)hipStreamSynchronize(st);
    T.free_all();
    g_tables.erase(key);
    return (int)ZK_ERR_DEVICE;
  };
  hipError_t e = hipSuccess;
  if (T.A == nullptr) {
    built = true;
    T.h = (log_n + 1) / 2;
    uint64_t nB = 1ull << T.h, nA = 1ull << (log_n - T.h);
    if ((e = tab_malloc(&T.A, nA * sizeof(UTab), &T.bytes)) != hipSuccess) return fail(e, "A");
    if ((e = tab_malloc(&T.B, nB * sizeof(UTab), &T.bytes)) != hipSuccess) return fail(e, "B");
    hipLaunchKernelGGL(ntt_pow_table_kernel, dim3((unsigned)((nA + 255) / 256)), dim3(256), 0, st, T.A, w, nB, nA);
    hipLaunchKernelGGL(ntt_pow_table_kernel, dim3((unsigned)((nB + 255) / 256)), dim3(256), 0, st, T.B, w, 1ull, nB);
    if ((e = hipGetLastError()) != hipSuccess) return fail(e, "launch");
  }
  if (want_roots) {
    for (int p = 0; p < nb; ++p) {
      uint32_t b = bs[p];
      if (b == 0 || T.roots[b] != nullptr) continue;
      built = true;
      uint64_t cnt = 1ull << (b - 1);
      if ((e = tab_malloc(&T.roots[b], cnt * sizeof(UTab), &T.bytes)) != hipSuccess) return fail(e, "roots");
      hipLaunchKernelGGL(ntt_pow_table_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, T.roots[b], w, 1ull << (log_n - b), cnt);
      if ((e = hipGetLastError()) != hipSuccess) return fail(e, "launch");
    }
  }
  if (full_log_s != 0 && (T.full == nullptr || T.full_log_s != full_log_s)) {
    if (T.full) {  // (another split of the same size: only when MI355ZK_NTT_LOGNP changes between calls)
      if ((e = hipDeviceSynchronize()) != hipSuccess) return fail(e, "sync");
      (void)hipFree(T.full);
      T.full = nullptr;
      T.bytes -= sizeof(UTab) << log_n;
    }
    built = true;
    const uint64_t cnt = 1ull << log_n;
    if ((e = tab_malloc(&T.full, cnt * sizeof(UTab), &T.bytes)) != hipSuccess) return fail(e, "full");
    T.full_log_s = full_log_s;
    hipLaunchKernelGGL(ntt_full_twiddle_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, st, T.full, T.A, T.B, T.h, full_log_s, cnt);
    if ((e = hipGetLastError()) != hipSuccess) return fail(e, "launch");
  }
  if (built && (e = hipStreamSynchronize(st)) != hipSuccess) return fail(e, "sync");  // one-time: tables may be used from other streams later
  *out = &T;
  return 0;
}

// The folded tables of (T's root, pre_g, post_c, post_g) (any of the three may be null, not all): found or built.  Called under g_run_mu;
// the device pointers are copied out before anybody can evict the entry.  with_full: the two-pass transform's full inter-pass table with
// everything that is constant per column / per row folded in (ntt_full_folded_kernel); otherwise (2^21 and up, no full table) the small
// tables of the same split: the first pass's stage table and pre^col, the last pass's (post^stride)^k and post_c * post^(row's first index),
// and for a transform scaled by post_c alone the low table of the two-level twiddle times post_c.
// bits[0 .. R): the passes' row lengths (log2), first pass first.
int build_folded(hipStream_t st, uint32_t log_n, const Fr& omega, PowTables* T, const PowTables* Tpre, const PowTables* Tpost, const Fr* pre_g, const Fr* post_c,
                 const TwU& post_cu, const Fr* post_g, const uint32_t* bits, int R, bool with_full, PowTables::Folded* out) {
  std::lock_guard<std::mutex> lk(g_mu);
  const uint32_t log_first = bits[0], log_last = bits[R - 1];
  const uint32_t log_s = log_n - log_first;             // columns of the first pass
  for (const auto& f : T->folded) {
    if (f.log_s != log_s || f.big != !with_full || f.has_pre != (pre_g != nullptr) || f.has_post_c != (post_c != nullptr) || f.has_post_g != (post_g != nullptr)) continue;
    if (pre_g && std::memcmp(&f.pre, pre_g, sizeof(Fr)) != 0) continue;
    if (post_c && std::memcmp(&f.post_c, post_c, sizeof(Fr)) != 0) continue;
    if (post_g && std::memcmp(&f.post_g, post_g, sizeof(Fr)) != 0) continue;
    *out = f;
    return 0;
  }
  if (T->folded.size() >= NTT_FOLDED_MAX) {   // the oldest goes, once nothing on the device can still be reading it
    ZK_HIP(hipDeviceSynchronize());
    T->folded.front().free_tabs();
    T->folded.erase(T->folded.begin());
  }
  PowTables::Folded f;
  f.log_s = log_s;
  f.big = !with_full;
  if (pre_g) { f.has_pre = true; f.pre = *pre_g; }
  if (post_c) { f.has_post_c = true; f.post_c = *post_c; }
  if (post_g) { f.has_post_g = true; f.post_g = *post_g; }
  const uint64_t cnt = 1ull << log_n, n_first = 1ull << log_first, n_cols = 1ull << log_s, n_last = 1ull << log_last, n_rows_last = cnt >> log_last;
  hipError_t e = hipSuccess;
  auto fail = [&](hipError_t err, const char* what) {
    std::fprintf(stderr, "[mi355zk] NTT folded-table build failed (%s): %s\n", what, hipGetErrorString(err));
    (void)hipStreamSynchronize(st);
    f.free_tabs();
    return (int)ZK_ERR_DEVICE;
  };
  auto grid = [](uint64_t c) { return dim3((unsigned)((c + 255) / 256)); };
  if (pre_g) {
    // i = x * n_cols + col:  pre^i = (pre^n_cols)^x * pre^col
    if ((e = tab_malloc(&f.pre_rows, n_first * sizeof(UTab), &f.bytes)) != hipSuccess) return fail(e, "pre rows");
    hipLaunchKernelGGL(ntt_pow_table_kernel, grid(n_first), dim3(256), 0, st, f.pre_rows, *pre_g, n_cols, n_first);
    if ((e = tab_malloc(&f.pre_stages, n_first * sizeof(UTab), &f.bytes)) != hipSuccess) return fail(e, "pre stages");
    hipLaunchKernelGGL(ntt_stage_table_kernel, grid(n_first), dim3(256), 0, st, f.pre_stages, *pre_g, n_cols, omega, n_cols, log_first);
    if (!with_full) {
      if ((e = tab_malloc(&f.pre_cols, n_cols * sizeof(UTab), &f.bytes)) != hipSuccess) return fail(e, "pre cols");
      hipLaunchKernelGGL(ntt_pow_table_kernel, grid(n_cols), dim3(256), 0, st, f.pre_cols, *pre_g, 1ull, n_cols);
    }
  }
  if (post_g) {
    // K = rb + n_rows_last * k (rb < n_rows_last the row's first output index):  post^K = post^rb * (post^n_rows_last)^k
    if ((e = tab_malloc(&f.post_rows, n_last * sizeof(UTab), &f.bytes)) != hipSuccess) return fail(e, "post rows");
    hipLaunchKernelGGL(ntt_pow_table_kernel, grid(n_last), dim3(256), 0, st, f.post_rows, *post_g, n_rows_last, n_last);
    if (!with_full) {
      if ((e = tab_malloc(&f.post_rowc, n_rows_last * sizeof(UTab), &f.bytes)) != hipSuccess) return fail(e, "post row constants");
      hipLaunchKernelGGL(ntt_pow_scaled_table_kernel, grid(n_rows_last), dim3(256), 0, st, f.post_rowc, *post_g, post_c ? *post_c : Fr::one(), n_rows_last);
    }
  } else if (post_c && !with_full) {
    const uint64_t nB = 1ull << T->h;
    if ((e = tab_malloc(&f.tw_b_scaled, nB * sizeof(UTab), &f.bytes)) != hipSuccess) return fail(e, "scaled twiddles");
    hipLaunchKernelGGL(ntt_pow_scaled_table_kernel, grid(nB), dim3(256), 0, st, f.tw_b_scaled, omega, *post_c, nB);
  }
  if (with_full) {
    if ((e = tab_malloc(&f.full, cnt * sizeof(UTab), &f.bytes)) != hipSuccess) return fail(e, "full");
    hipLaunchKernelGGL(ntt_full_folded_kernel, grid(cnt), dim3(256), 0, st, f.full, T->A, T->B, T->h, log_s, cnt,
                       Tpre ? Tpre->A : nullptr, Tpre ? Tpre->B : nullptr, Tpre ? Tpre->h : 0u, Tpost ? Tpost->A : nullptr,
                       Tpost ? Tpost->B : nullptr, Tpost ? Tpost->h : 0u, post_cu, post_c != nullptr ? 1 : 0);
  }
  if ((e = hipGetLastError()) != hipSuccess) return fail(e, "launch");
  if ((e = hipStreamSynchronize(st)) != hipSuccess) return fail(e, "sync");   // one-time: the tables may be used from other streams later
  T->folded.push_back(f);
  *out = f;
  return 0;
}

// The inter-pass scratch, one array per (device, stream) and bounded (device_mem.hpp: StreamScratch).  Guarded by g_run_mu, which every
// transform holds while launching: that keeps other transforms from being enqueued while the scratch drops a device's buffers.
StreamScratch g_scratch;
std::mutex g_run_mu;
int scratch_for(int dev, hipStream_t st, size_t bytes, Fr** out) { return g_scratch.get(dev, st, bytes, (void**)out); }

// host: a Montgomery form -> the plain integer and its quotient.  The quotient is a 261-round division (~10 us on the host): the few
// scale factors a process uses (1/m per domain size) are kept.  Called under g_run_mu.
static TwU to_tw(const Fr& x) {
  static std::vector<std::pair<Fr, TwU>> memo;
  for (const auto& e : memo)
    if (std::memcmp(&e.first, &x, sizeof(Fr)) == 0) return e.second;
  const TwU t = tw_make(to_canonical(x));
  if (memo.size() >= 64) memo.clear();
  memo.emplace_back(x, t);
  return t;
}

}  // namespace

void ntt_release_all() {
  std::lock_guard<std::mutex> lk2(g_run_mu);  // (same order as the run path: g_run_mu, then g_mu)
  std::lock_guard<std::mutex> lk(g_mu);
  for (auto& kv : g_tables) {
    (void)hipSetDevice(kv.first.dev);
    kv.second.free_all();
  }
  g_tables.clear();
  g_scratch.release_all();
}

}  // namespace zk
