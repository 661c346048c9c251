// The NTT's host arithmetic without a device (tests/test_ntt_plan_host.py): the planner (ntt_plan.hpp), compiled by the host compiler alone.
//   test_ntt_host plan   invariants of every plan of the grid under the default knobs and every knob setting below + one case per argument
//                        error; prints "ok <cases>" or FAIL lines
//   test_ntt_host dump   every planned value of the grid, one line per request (knobs from the environment, as the library reads them);
//                        table sources are spelled as names
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../phase2-bn254_amd/csrc/ntt_plan.hpp"

using namespace zk;

// ---------------------------------------------------------------- the grid of requests
static std::vector<NttRequest> grid() {
  std::vector<NttRequest> out;
  for (uint32_t log_n = 1; log_n <= 30; ++log_n)
    for (uint32_t batch : {1u, 3u, 8u})
      for (int m = 0; m < 8; ++m) {
        NttRequest Q;
        Q.log_n = log_n;
        Q.batch = batch;
        Q.pre_g = m & 1;
        Q.post_c = m & 2;
        Q.post_g = m & 4;
        out.push_back(Q);
      }
  return out;
}

// the knob settings profiles/ntt_host_split.md compares with the parent, as the structs ntt_knobs() makes of them
static std::vector<std::pair<std::string, NttKnobs>> settings() {
  std::vector<std::pair<std::string, NttKnobs>> out;
  auto add = [&](const char* name, auto&& set) {
    NttKnobs K;
    set(K);
    out.emplace_back(name, K);
  };
  add("default", [](NttKnobs&) {});
  add("LOGNP=10", [](NttKnobs& K) { K.lognp = 10; });
  add("LOGNP=11", [](NttKnobs& K) { K.lognp = 11; });
  add("LOGNP=12", [](NttKnobs& K) { K.lognp = 12; });
  add("TILE=1024", [](NttKnobs& K) { K.tile = 1024; });
  add("TILE=2048", [](NttKnobs& K) { K.tile = 2048; });
  add("TILE=4096", [](NttKnobs& K) { K.tile = 4096; });
  add("RADIX=2", [](NttKnobs& K) { K.radix = 2; });
  add("RADIX=4", [](NttKnobs& K) { K.radix = 4; });
  add("WAVELOCAL=0", [](NttKnobs& K) { K.no_wavelocal = true; });
  add("NO_FULL_TW", [](NttKnobs& K) { K.no_full_tw = true; });
  add("NO_FOLD", [](NttKnobs& K) { K.no_fold = true; });
  add("NO_STAGE_FOLD", [](NttKnobs& K) { K.no_stage_fold = true; });
  add("NOPAIR", [](NttKnobs& K) { K.no_pair = true; });
  add("PAIR=1", [](NttKnobs& K) { K.pair = 1; });
  add("PAIR_ALL", [](NttKnobs& K) { K.pair_all = true; });
  return out;
}

static const char* const ARG_NAMES[NTT_ARGS] = {"twA", "twB", "preA", "preB", "postA", "postB", "twF"};

static void dump(const NttRequest& Q, int rc, const NttPlan& N) {
  std::printf("log_n=%u batch=%u pre_g=%d post_c=%d post_g=%d: rc=%d", Q.log_n, Q.batch, (int)Q.pre_g, (int)Q.post_c, (int)Q.post_g, rc);
  if (rc) { std::printf("\n"); return; }
  std::printf(" R=%d b=", N.R);
  for (int p = 0; p < N.R; ++p) std::printf("%s%u", p ? "," : "", N.b[p]);
  std::printf(" h=%u full_tw=%d fold=%d fold_big=%d full_log_s=%u Tpre=%d Tpost=%d F=%d with_full=%d members=", N.h, (int)N.full_tw, (int)N.fold, (int)N.fold_big,
              N.full_log_s, (int)N.want_tpre, (int)N.want_tpost, (int)N.want_folded, (int)(N.want_folded && N.fold));
  bool any = false;
  for (uint32_t t = 0; t < NTT_TAB_COUNT; ++t)
    if (N.folded_members >> t & 1) { std::printf("%s%s", any ? "+" : "", ntt_tab_name((NttTab)t)); any = true; }
  if (!any) std::printf("-");
  std::printf(" scratch_bytes=%" PRIu64, N.want_scratch ? ((uint64_t)sizeof(Fr) << Q.log_n) * Q.batch : (uint64_t)0);
  for (int p = 0; p < N.R; ++p) {
    const NttPass& s = N.pass[p];
    const NttPassParams& P = s.P;
    if (s.kind == NTT_KERNEL_WL) std::printf(" | pass=%d kernel=(ntt_pass_wl_kernel<%u>)", p, P.log_np);
    else std::printf(" | pass=%d kernel=(ntt_pass_kernel<%u, %s>)", p, P.log_np, s.kind == NTT_KERNEL_R4 ? "true" : "false");
    std::printf(" grid=%u threads=%u lds=%zu src=%s dst=%s", s.grid, s.threads, s.lds_bytes, s.src == NTT_BUF_ARRAY ? "array" : "scratch",
                s.dst == NTT_BUF_ARRAY ? "array" : "scratch");
    std::printf(" P=%u,%u,%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%u,%" PRIu64 ",%u,%u,%u,%u,%u,%u,%u,%u,%" PRIu64,
                P.log_np, P.g, P.in_xs, P.in_gs, P.out_xs, P.out_gs, P.tiles_lo, P.in_hi_stride, P.in_lo_stride, P.out_hi_stride, P.out_lo_stride, P.load_x_fastest,
                P.tw_mul, P.tw_h, P.tw_full, P.pre, P.pre_h, P.post, P.post_h, P.xcd_pair, P.batch, P.tiles);
    std::printf(" roots=T.roots[%u]", P.log_np);
    for (uint32_t a = 0; a < NTT_ARGS; ++a) std::printf(" %s=%s", ARG_NAMES[a], ntt_tab_name(s.tab[a]));
  }
  std::printf("\n");
}

// ---------------------------------------------------------------- plan invariants
static int g_fail = 0;
static const char* g_setting = "";
#define CHECK(cond)                                                                                            \
  do {                                                                                                         \
    if (!(cond)) { ++g_fail; std::printf("FAIL [%s] %s (line %d): ", g_setting, #cond, __LINE__); dump(Q, 0, N); } \
  } while (0)

// the kernels' tile permutation (ntt_pass_kernel / ntt_pass_wl_kernel: P.xcd_pair)
static uint64_t permute_tile(uint64_t tile, uint32_t xcd_pair) {
  if (xcd_pair == 1) return (tile & ~15ull) | ((tile & 7ull) << 1) | ((tile >> 3) & 1ull);
  if (xcd_pair == 5) return (tile & ~255ull) | ((tile & 7ull) << 5) | ((tile >> 3) & 31ull);
  return tile;
}

// (stride, count) digits address [0, n) exactly once iff, sorted by stride, each stride is the product of the counts below it
static bool mixed_radix(std::vector<std::pair<uint64_t, uint64_t>> d, uint64_t n) {
  d.erase(std::remove_if(d.begin(), d.end(), [](const std::pair<uint64_t, uint64_t>& x) { return x.second == 1; }), d.end());
  std::sort(d.begin(), d.end());
  uint64_t prod = 1;
  for (const auto& x : d) {
    if (x.second == 0 || x.first != prod) return false;
    prod *= x.second;
  }
  return prod == n;
}

static void check_plan(const NttRequest& Q, const NttKnobs& K, const NttPlan& N) {
  const uint64_t n = 1ull << Q.log_n;
  const int R = N.R;
  CHECK(R >= 1 && R <= 3);
  if (R < 1 || R > 3) return;
  uint32_t sum = 0;
  for (int p = 0; p < R; ++p) {
    CHECK(N.b[p] >= 1 && N.b[p] <= 12);
    sum += N.b[p];
  }
  CHECK(sum == Q.log_n);
  CHECK(N.h == (Q.log_n + 1) / 2);
  CHECK(!(N.fold && N.fold_big) && (!N.fold || N.full_tw) && (!N.fold_big || !N.full_tw));
  CHECK(N.want_folded == (N.fold || N.fold_big) && (N.want_folded || N.folded_members == 0));
  CHECK((N.full_log_s != 0) == (N.full_tw && !N.fold) && (N.full_log_s == 0 || N.full_log_s == N.b[1]));
  CHECK(N.want_tpre == Q.pre_g && N.want_tpost == Q.post_g);
  CHECK(N.want_scratch == (R > 1));
  // what each knob promises, whatever the request
  if (K.lognp) {
    const uint32_t want_r = (Q.log_n + (uint32_t)K.lognp - 1) / (uint32_t)K.lognp;   // rows of at most 2^lognp, as few passes as that allows
    CHECK((uint32_t)R == want_r);
    for (int p = 0; p < R; ++p) CHECK(N.b[p] <= (uint32_t)K.lognp);
  }
  if (K.no_full_tw) CHECK(!N.full_tw && !N.fold && N.full_log_s == 0);
  if (K.no_fold) CHECK(!N.want_folded && !N.fold && !N.fold_big && N.folded_members == 0);
  for (int p = 0; p < R; ++p) {
    const NttPass& s = N.pass[p];
    const uint64_t elems = (uint64_t)s.P.g << s.P.log_np;
    if (K.tile) CHECK(elems <= (uint64_t)K.tile || s.P.g == 1);        // a tile holds at most `tile` elements, or one row longer than that
    if (K.radix == 2) CHECK(s.kind == NTT_KERNEL_R2);
    if (K.radix == 4) CHECK(s.kind != NTT_KERNEL_R2);
    if (K.no_wavelocal) CHECK(s.kind != NTT_KERNEL_WL);
    if (K.no_pair) CHECK(s.P.xcd_pair == 0);
    if (s.P.xcd_pair != 0) CHECK(s.P.xcd_pair == K.pair && (K.pair_all || s.P.g <= 2));
    if (K.no_stage_fold) CHECK(s.P.pre != 3);
    if (K.no_fold) CHECK(s.P.pre <= 1 && (s.P.post == 0 || s.P.post <= 3));
    for (uint32_t a = 0; a < NTT_ARGS; ++a) {
      if (K.no_fold) CHECK(!ntt_tab_is_folded(s.tab[a]));
      if (K.no_full_tw) CHECK(s.tab[a] != NTT_TAB_T_FULL && s.tab[a] != NTT_TAB_F_FULL);
    }
  }

  std::vector<uint8_t> seen;
  for (int p = 0; p < R; ++p) {
    const NttPass& s = N.pass[p];
    const NttPassParams& P = s.P;
    const bool first = p == 0, last = p == R - 1;
    const uint64_t np = 1ull << P.log_np, elems = (uint64_t)P.g * np;
    CHECK(P.log_np == N.b[p] && P.g >= 1 && P.batch == Q.batch);
    // launch geometry
    CHECK(s.lds_bytes == elems * 36 && s.lds_bytes <= NTT_LDS_BYTES_MAX);
    CHECK(s.threads >= 64 && s.threads <= 1024);
    CHECK(s.kind < NTT_KERNEL_KINDS);
    if (s.kind == NTT_KERNEL_WL) CHECK(elems == 4ull * s.threads && P.log_np >= 8);
    CHECK(P.tiles * Q.batch <= 0xffffffffull && s.grid == P.tiles * Q.batch);
    CHECK(P.xcd_pair == 0 || P.tiles % 256 == 0);   // otherwise the kernel's tile permutation is no bijection
    // source and destination
    CHECK(s.src == (first ? NTT_BUF_ARRAY : NTT_BUF_SCRATCH) && s.dst == (last ? NTT_BUF_ARRAY : NTT_BUF_SCRATCH));

    // coverage: loads and stores of the pass are permutations of [0, n)
    CHECK(P.tiles_lo >= 1 && P.tiles % P.tiles_lo == 0 && P.tiles * elems == n);
    if (P.tiles_lo == 0 || P.tiles % P.tiles_lo != 0) continue;
    const uint64_t tiles_hi = P.tiles / P.tiles_lo;
    CHECK(mixed_radix({{P.in_hi_stride, tiles_hi}, {P.in_lo_stride, P.tiles_lo}, {P.in_xs, np}, {P.in_gs, P.g}}, n));
    CHECK(mixed_radix({{P.out_hi_stride, tiles_hi}, {P.out_lo_stride, P.tiles_lo}, {P.out_xs, np}, {P.out_gs, P.g}}, n));
    if (Q.log_n <= 16 && P.tiles * elems == n) {
      for (int store = 0; store < 2; ++store) {
        seen.assign(n, 0);
        bool ok = true;
        for (uint64_t t = 0; t < P.tiles && ok; ++t) {
          const uint64_t tile = permute_tile(t, P.xcd_pair);
          const uint64_t hi = tile / P.tiles_lo, lo = tile % P.tiles_lo;
          const uint64_t base = store ? hi * P.out_hi_stride + lo * P.out_lo_stride : hi * P.in_hi_stride + lo * P.in_lo_stride;
          for (uint64_t g = 0; g < P.g && ok; ++g)
            for (uint64_t x = 0; x < np; ++x) {
              const uint64_t a = base + x * (store ? P.out_xs : P.in_xs) + g * (store ? P.out_gs : P.in_gs);
              if (a >= n || seen[a]++) { ok = false; break; }
            }
        }
        CHECK(ok);   // (every address below n and none twice: n addresses, so all of [0, n))
      }
    }

    // the inter-pass twiddle: every pass but the last multiplies one in, from the full table or the two-level pair
    CHECK((P.tw_full != 0) == (N.full_tw && first) && (P.tw_full == 0 || R == 2));
    CHECK(last ? P.tw_mul == 0 : P.tw_mul != 0);
    if (P.tw_full) CHECK(s.tab[NTT_ARG_TW_F] == (N.fold ? NTT_TAB_F_FULL : NTT_TAB_T_FULL));
    if (P.tw_mul && !P.tw_full) CHECK(s.tab[NTT_ARG_TW_A] == NTT_TAB_T_A && (s.tab[NTT_ARG_TW_B] == NTT_TAB_T_B || s.tab[NTT_ARG_TW_B] == NTT_TAB_F_TW_B_SCALED) && P.tw_h == N.h);

    // table consistency: every table a pass names is among the plan's requests
    for (uint32_t a = 0; a < NTT_ARGS; ++a) {
      const NttTab t = s.tab[a];
      CHECK(t < NTT_TAB_COUNT);
      if (ntt_tab_is_folded(t)) CHECK(N.want_folded && (N.folded_members >> t & 1));
      if (t == NTT_TAB_F_FULL) CHECK(N.fold);
      if (t == NTT_TAB_T_FULL) CHECK(N.full_tw && !N.fold && N.full_log_s != 0);
      if (t == NTT_TAB_TPRE_A || t == NTT_TAB_TPRE_B) CHECK(N.want_tpre);
      if (t == NTT_TAB_TPOST_A || t == NTT_TAB_TPOST_B) CHECK(N.want_tpost);
    }
    // ... and the tables behind each scale mode are the ones its kernel branch reads
    const NttTab preA = s.tab[NTT_ARG_PRE_A], preB = s.tab[NTT_ARG_PRE_B], postA = s.tab[NTT_ARG_POST_A], postB = s.tab[NTT_ARG_POST_B];
    CHECK((P.pre != 0) == (first && Q.pre_g));
    CHECK((P.post != 0) == last);
    if (P.pre == 1) CHECK(preA == NTT_TAB_TPRE_A && preB == NTT_TAB_TPRE_B && P.pre_h == N.h && !N.fold);
    if (P.pre == 2) CHECK(preA == NTT_TAB_F_PRE_ROWS && N.fold);
    if (P.pre == 3) CHECK(preA == NTT_TAB_F_PRE_STAGES && N.fold && s.kind == NTT_KERNEL_WL);
    if (P.pre == 4) CHECK(preA == NTT_TAB_F_PRE_STAGES && preB == NTT_TAB_F_PRE_COLS && N.fold_big && s.kind == NTT_KERNEL_WL);
    CHECK(P.pre <= 4);
    if (P.post == 2) CHECK(postA == NTT_TAB_TPOST_A && postB == NTT_TAB_TPOST_B && P.post_h == N.h && !N.fold);
    if (P.post == 4) CHECK(postA == NTT_TAB_F_POST_ROWS && N.fold);
    if (P.post == 5) CHECK(postA == NTT_TAB_F_POST_ROWS && postB == NTT_TAB_F_POST_ROWC && N.fold_big && s.kind == NTT_KERNEL_WL);
    CHECK(P.post <= 5);
    // the barrier kernels receive the unshadowed pre / post tables (they know neither the stage table nor the row constants)
    if (s.kind != NTT_KERNEL_WL) {
      CHECK(preA == (!Q.pre_g ? NTT_TAB_NULL : N.fold ? NTT_TAB_F_PRE_ROWS : NTT_TAB_TPRE_A) && preB == (Q.pre_g && !N.fold ? NTT_TAB_TPRE_B : NTT_TAB_NULL));
      CHECK(postA == (!Q.post_g ? NTT_TAB_NULL : N.fold ? NTT_TAB_F_POST_ROWS : NTT_TAB_TPOST_A) && postB == (Q.post_g && !N.fold ? NTT_TAB_TPOST_B : NTT_TAB_NULL));
    }
    // post_c riding on the scaled low twiddle table: only in the pass before the last, only for a transform scaled by post_c alone
    if (s.tab[NTT_ARG_TW_B] == NTT_TAB_F_TW_B_SCALED) CHECK(p == R - 2 && N.fold_big && Q.post_c && !Q.post_g && N.pass[R - 1].P.post == 3);
  }
  // the last pass multiplies by nothing exactly when nothing is left to multiply there
  const bool rides = R >= 2 && N.pass[R - 2].tab[NTT_ARG_TW_B] == NTT_TAB_F_TW_B_SCALED;
  const bool nothing_left = (!Q.post_c && !Q.post_g) || (N.fold && !Q.post_g) || rides;
  CHECK((N.pass[R - 1].P.post == 3) == nothing_left);
  if (N.fold_big && Q.post_c && !Q.post_g) CHECK(rides);   // (otherwise post_c would be multiplied in by nobody or twice)
  if (!nothing_left && !Q.post_g) CHECK(N.pass[R - 1].P.post == 1);
}

static int run_plan() {
  int cases = 0;
  const std::vector<NttRequest> G = grid();
  for (const auto& s : settings()) {
    g_setting = s.first.c_str();
    for (const NttRequest& Q : G) {
      NttPlan N;
      const int rc = ntt_plan(Q, s.second, &N);
      if (rc != ZK_OK) { ++g_fail; std::printf("FAIL [%s] refused: ", g_setting); dump(Q, rc, N); continue; }
      check_plan(Q, s.second, N);
      ++cases;
    }
  }
  // one refused request per argument check (the third refusal, a row length with no kernel, cannot be reached from any request: rows are 1 .. 12 bits;
  // log_n == 0 is no refusal: the launcher's early exit, no pass to plan)
  g_setting = "refusals";
  auto refused = [&](uint32_t log_n, uint32_t batch) {
    NttRequest Q;
    Q.log_n = log_n;
    Q.batch = batch;
    NttPlan N{};
    const int rc = ntt_plan(Q, NttKnobs{}, &N);
    if (rc != ZK_ERR_BAD_ARGS) { ++g_fail; std::printf("FAIL not refused with rc 3: "); dump(Q, rc, N); }
    ++cases;
  };
  refused(10, 0);
  refused(10, NTT_MAX_BATCH + 1);
  refused(31, 1);
  if (g_fail) { std::printf("FAILED %d checks\n", g_fail); return 1; }
  std::printf("ok %d\n", cases);
  return 0;
}

int main(int argc, char** argv) {
  if (argc >= 2 && std::strcmp(argv[1], "plan") == 0) return run_plan();
  if (argc >= 2 && std::strcmp(argv[1], "dump") == 0) {
    for (const NttRequest& Q : grid()) {
      NttPlan N{};
      const int rc = ntt_plan(Q, ntt_knobs(), &N);
      dump(Q, rc, N);
    }
    return 0;
  }
  std::fprintf(stderr, "usage: test_ntt_host plan | dump\n");
  return 2;
}
