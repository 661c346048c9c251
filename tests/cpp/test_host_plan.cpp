// The host-buffer entry points' host arithmetic without a device (tests/test_host_plan_host.py): host_plan.hpp compiled by the host compiler alone.
//   test_host_plan plan   invariants of the density plan, the chunk schedule, the cells, the join and the small planners over the grids
//                         below; prints "ok <cases>" or FAIL lines
//   test_host_plan dump   every planned value of the cut, cell, join and weight grids, one line per case (knobs from the environment, as
//                         the library reads them); no pointer values
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../phase2-bn254_amd/csrc/host_plan.hpp"

using namespace zk;

// ---------------------------------------------------------------- what is under test, behind four plain functions
static std::vector<uint64_t> cuts_of(uint64_t n, bool upload_bases) { return host_chunk_cuts(n, upload_bases, host_knobs()); }
static CellPlan cells_of(const DensityPlan& P, uint64_t base_offset, size_t n_devices) { return plan_cells(P, base_offset, n_devices, host_knobs(), msm_knobs()); }
static CellJoin join_of(const int* rc, const long long* err, const uint64_t* lo, size_t count, long long eof) { return join_cells(rc, err, lo, count, eof); }
static std::vector<size_t> wcuts_of(const uint32_t* row_ptr, size_t n_rows, size_t nnz, size_t devices) {
  return weight_cuts(row_ptr, n_rows, nnz, range_parts(n_rows, devices, 128));
}

// ---------------------------------------------------------------- helpers
static long g_cases = 0;
static int g_fail = 0;
#define CHECK(cond, ...)                          \
  do {                                            \
    if (!(cond)) {                                \
      if (++g_fail <= 40) {                       \
        std::printf("FAIL %s (line %d): ", #cond, __LINE__); \
        std::printf(__VA_ARGS__);                 \
        std::printf("\n");                        \
      }                                           \
    }                                             \
  } while (0)

static const char* KNOBS[] = {"MI355ZK_HOST_CHUNK_GROWTH", "MI355ZK_HOST_CHUNK_FIRST", "MI355ZK_HOST_CHUNK_TEST",
                              "MI355ZK_MULTI_PLAN",        "MI355ZK_MULTI_MIN_LOG",    "MI355ZK_DENSE_PIECE_TEST"};
static void set_knob(const char* name, const char* value) {  // every knob of host_knobs() unset but this one (nullptr: all unset)
  for (const char* k : KNOBS) unsetenv(k);
  if (name) setenv(name, value, 1);
}

struct Rng {  // splitmix64
  uint64_t s;
  uint64_t next() {
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
  }
};
// a density map of at least `bits` bits (and a spare word): kind 0 all ones, 1 all zero, 2 random with seed 1; the bits past `bits` are
// set the same way (the plan must not look at them)
static std::vector<uint32_t> make_map(uint64_t bits, int kind, uint64_t seed = 1) {
  std::vector<uint32_t> m((bits + 31) / 32 + 1);
  Rng r{seed};
  for (auto& w : m) w = kind == 0 ? 0xffffffffu : kind == 1 ? 0u : (uint32_t)r.next();
  return m;
}
static bool bit(const std::vector<uint32_t>& m, uint64_t i) { return (m[i >> 5] >> (i & 31)) & 1u; }

// ---------------------------------------------------------------- density
static void check_density() {
  for (uint64_t n : {0ull, 1ull, 31ull, 32ull, 33ull, 70ull, 1000ull})
    for (int bits_kind = 0; bits_kind < 3; ++bits_kind)     // density_bits shorter than, equal to, longer than n_scalars
      for (int kind = 0; kind < 4; ++kind)                  // all ones, all zero, random, FullDensity
        for (int eof_kind = 0; eof_kind < 3; ++eof_kind)    // the bases run out before / inside / after the selected exponents
          for (uint64_t base_offset : {0ull, 3ull}) {
            const uint64_t bits = bits_kind == 0 ? n / 2 : bits_kind == 1 ? n : n + 40;
            const bool full = kind == 3;
            const std::vector<uint32_t> map = make_map(bits > n ? bits : n, full ? 0 : kind);
            const uint64_t nn = full ? n : (bits < n ? bits : n);
            uint64_t total = 0;
            for (uint64_t i = 0; i < nn; ++i) total += full || bit(map, i);
            const uint64_t avail = eof_kind == 0 ? 0 : eof_kind == 1 ? total / 2 : total + 5;
            // (base_offset 3 with no base available: an offset PAST the vector)
            const uint64_t n_bases = avail == 0 && base_offset ? 1 : base_offset + avail;
            const DensityPlan P = plan_density(n_bases, base_offset, n, full ? nullptr : map.data(), bits);
            ++g_cases;
            CHECK(P.n == nn, "n=%" PRIu64 " bits=%" PRIu64 " kind=%d: P.n=%" PRIu64, n, bits, kind, P.n);
            // bit-by-bit: rank, select, the first exponent without a base
            long long eof = -1;
            uint64_t r = 0;
            for (uint64_t i = 0; i <= nn; ++i) {
              CHECK(P.rank(i) == r, "n=%" PRIu64 " bits=%" PRIu64 " kind=%d: rank(%" PRIu64 ")=%" PRIu64 " want %" PRIu64, n, bits, kind, i, P.rank(i), r);
              if (i == nn) break;
              if (full || bit(map, i)) {
                CHECK(P.select(r) == i, "n=%" PRIu64 " bits=%" PRIu64 " kind=%d: select(%" PRIu64 ")=%" PRIu64 " want %" PRIu64, n, bits, kind, r, P.select(r), i);
                CHECK(P.select(P.rank(i)) == i, "select(rank(%" PRIu64 "))", i);
                if (eof < 0 && r >= avail) eof = (long long)i;
                ++r;
              }
            }
            CHECK(r == total, "total");
            if (!full) CHECK(P.select(total) == nn, "n=%" PRIu64 " kind=%d: select(total)=%" PRIu64 " want %" PRIu64, n, kind, P.select(total), nn);
            CHECK(P.eof_index == eof, "n=%" PRIu64 " bits=%" PRIu64 " kind=%d avail=%" PRIu64 ": eof=%lld want %lld", n, bits, kind, avail, P.eof_index, eof);
            CHECK(P.live() == (eof >= 0 ? (uint64_t)eof : nn), "live");
          }
}

// ---------------------------------------------------------------- chunk cuts
static const uint64_t CUT_N[] = {0, 1, 1ull << 21, (1ull << 23) - 32, 1ull << 23, (1ull << 24) + 40, 1ull << 26};
static const struct { const char* name; const char* value; } CUT_SETTINGS[] = {
    {nullptr, nullptr}, {"MI355ZK_HOST_CHUNK_TEST", "64"}, {"MI355ZK_HOST_CHUNK_TEST", "512"}, {"MI355ZK_HOST_CHUNK_FIRST", "22"}, {"MI355ZK_HOST_CHUNK_GROWTH", "150"}};

static void check_cuts() {
  for (const auto& s : CUT_SETTINGS) {
    set_knob(s.name, s.value);
    const bool test_knob = s.name && std::strstr(s.name, "CHUNK_TEST");
    for (uint64_t n : CUT_N)
      for (int up = 0; up < 2; ++up) {
        const std::vector<uint64_t> c = cuts_of(n, up != 0);
        ++g_cases;
        if (n == 0) { CHECK(c.size() == 1 && c[0] == 0, "n=0: %zu cuts", c.size()); continue; }   // no chunk
        CHECK(c.size() >= 2 && c.front() == 0 && c.back() == n, "n=%" PRIu64 ": ends", n);
        for (size_t i = 1; i < c.size(); ++i) {
          CHECK(c[i] > c[i - 1], "n=%" PRIu64 ": cut %zu not increasing", n, i);
          if (i + 1 < c.size()) CHECK(c[i] % 32 == 0, "n=%" PRIu64 ": inner cut %" PRIu64, n, c[i]);
        }
        if (!test_knob && n < 4 * (1ull << 21)) CHECK(c.size() == 2, "n=%" PRIu64 ": %zu chunks below the threshold", n, c.size() - 1);
        if (test_knob) CHECK(c.size() - 1 == (n + (uint64_t)std::atoi(s.value) - 1) / (uint64_t)std::atoi(s.value), "n=%" PRIu64 ": test chunks", n);
      }
  }
  set_knob(nullptr, nullptr);
}

// ---------------------------------------------------------------- cells
static const uint64_t CELL_N[] = {64, 100, 4096, (1ull << 20) + 17};
static const size_t CELL_DEVS[] = {1, 2, 3, 8};
static const char* CELL_PLANS[] = {nullptr, "2x1", "1x2", "2x2", "9x9", "0x1"};
constexpr uint64_t CELL_BASE_OFFSET = 5;

// the call of a cell case: FullDensity with a base for every exponent, or a random map whose last three selected exponents have no base
struct CellCase {
  std::vector<uint32_t> map;
  DensityPlan P;
  uint64_t n_bases;
};
static CellCase cell_case(uint64_t n, bool with_map) {
  CellCase c;
  if (!with_map) {
    c.n_bases = CELL_BASE_OFFSET + n;
    c.P = plan_density(c.n_bases, CELL_BASE_OFFSET, n, nullptr, 0);
    return c;
  }
  c.map = make_map(n, 2, 1 + n);
  uint64_t total = 0;
  for (uint64_t i = 0; i < n; ++i) total += bit(c.map, i);
  c.n_bases = CELL_BASE_OFFSET + total - 3;
  c.P = plan_density(c.n_bases, CELL_BASE_OFFSET, n, c.map.data(), n);
  return c;
}

static void check_cells() {
  for (const char* plan : CELL_PLANS) {
    set_knob(plan ? "MI355ZK_MULTI_PLAN" : nullptr, plan);
    unsigned a = 0, b = 0;
    const bool asked = plan && std::sscanf(plan, "%ux%u", &a, &b) == 2;
    for (uint64_t n : CELL_N)
      for (size_t devs : CELL_DEVS)
        for (int with_map = 0; with_map < 2; ++with_map) {
          const CellCase cc = cell_case(n, with_map != 0);
          const DensityPlan& P = cc.P;
          const uint64_t live = P.live();
          const CellPlan C = cells_of(P, CELL_BASE_OFFSET, devs);
          ++g_cases;
          const char* pl = plan ? plan : "-";
          CHECK(with_map ? (P.eof_index >= 0 && live < n) : live == n, "the case itself");
          // an impossible plan (more cells than devices, a zero) falls back to one range per device; a possible one is taken as asked, and
          // then only shrinks: window groups to 1 when the window count does not divide, ranges while one would be shorter than 32
          const bool possible = asked && a >= 1 && b >= 1 && (size_t)a * b <= devs;
          const uint32_t pg0 = possible ? a : (uint32_t)devs, wg0 = possible ? b : 1;
          CHECK(C.pg >= 1 && C.pg <= pg0 && (C.wg == wg0 || C.wg == 1), "n=%" PRIu64 " devs=%zu plan=%s: pg=%u wg=%u", n, devs, pl, C.pg, C.wg);
          if (live / pg0 >= 64) CHECK(C.pg == pg0, "n=%" PRIu64 " devs=%zu plan=%s: pg=%u shrank", n, devs, pl, C.pg);
          if (C.wg > 1) {
            const uint32_t W = choose_geom((live + pg0 - 1) / pg0, 1, C.wg, msm_knobs()).W;
            CHECK(W && W % C.wg == 0, "n=%" PRIu64 " plan=%s: %u windows in %u groups", n, pl, W, C.wg);
          }
          // the ranges tile [0, live), inner cuts multiples of 32, every range of at least 32 exponents unless it is the only one
          CHECK(C.cut.size() == (size_t)C.pg + 1 && C.cut.front() == 0 && C.cut.back() == live, "n=%" PRIu64 " devs=%zu plan=%s: ends", n, devs, pl);
          for (uint32_t r = 0; r < C.pg; ++r) {
            CHECK(C.cut[r + 1] >= C.cut[r], "order");
            if (r) CHECK(C.cut[r] % 32 == 0, "n=%" PRIu64 " devs=%zu plan=%s: inner cut %" PRIu64, n, devs, pl, C.cut[r]);
            if (C.pg > 1) CHECK(C.cut[r + 1] - C.cut[r] >= 32, "n=%" PRIu64 " live=%" PRIu64 " devs=%zu plan=%s: range %u holds %" PRIu64, n, live, devs, pl, r, C.cut[r + 1] - C.cut[r]);
          }
          // the cells: every non-empty range once per window group, in order, dealt to the device slots in turn; base slices contiguous and
          // inside [base_offset, n_bases)
          size_t k = 0;
          uint64_t next_base = CELL_BASE_OFFSET;
          for (uint32_t r = 0; r < C.pg; ++r) {
            if (C.cut[r + 1] == C.cut[r]) continue;
            for (uint32_t g = 0; g < C.wg; ++g, ++k) {
              if (k >= C.cells.size()) break;
              const HostCell& c = C.cells[k];
              CHECK(c.lo == C.cut[r] && c.hi == C.cut[r + 1] && c.wgi == g && c.slot == k % devs, "n=%" PRIu64 " devs=%zu plan=%s: cell %zu", n, devs, pl, k);
              CHECK(c.boff == next_base && c.boff >= CELL_BASE_OFFSET && c.boff + c.used <= cc.n_bases, "n=%" PRIu64 " devs=%zu plan=%s: cell %zu slice %" PRIu64 "+%" PRIu64, n, devs, pl, k, c.boff, c.used);
              uint64_t sel = 0;
              if (n <= 4096) { for (uint64_t i = c.lo; i < c.hi; ++i) sel += !with_map || bit(cc.map, i); CHECK(sel == c.used, "cell %zu uses %" PRIu64 " bases, %" PRIu64 " selected", k, c.used, sel); }
            }
            if (k && k <= C.cells.size()) next_base = C.cells[k - 1].boff + C.cells[k - 1].used;
          }
          CHECK(k == C.cells.size(), "n=%" PRIu64 " devs=%zu plan=%s: %zu cells, %zu expected", n, devs, pl, C.cells.size(), k);
          CHECK(next_base == CELL_BASE_OFFSET + P.rank(live), "the slices end at the last consumed base");
        }
  }
  set_knob(nullptr, nullptr);
}

// ---------------------------------------------------------------- join
// the outcomes of one cell: OK, bad arguments with / without an index, identity, device error, and a code a cell cannot return (Eof)
enum { O_OK, O_BAD_IDX, O_BAD, O_IDENT, O_DEV, O_ODD, N_OUTCOMES };
static const int OUTCOME_RC[N_OUTCOMES] = {ZK_OK, ZK_ERR_BAD_ARGS, ZK_ERR_BAD_ARGS, ZK_ERR_UNEXPECTED_IDENTITY, ZK_ERR_DEVICE, ZK_ERR_UNEXPECTED_EOF};
struct JoinCase {
  int rc[3];
  long long err[3];
  uint64_t lo[3];
  long long eof;
};
template <class Fn>
static void for_join_cases(Fn&& fn) {
  const uint64_t lo[3] = {0, 32, 64};
  // local error indices: rising and falling with the cell (so that the lowest GLOBAL index is not always the first cell's), and equal globals
  const long long errs[3][3] = {{3, 5, 7}, {70, 5, 0}, {40, 8, 8}};
  for (int o0 = 0; o0 < N_OUTCOMES; ++o0)
    for (int o1 = 0; o1 < N_OUTCOMES; ++o1)
      for (int o2 = 0; o2 < N_OUTCOMES; ++o2)
        for (const auto& e : errs)
          for (long long eof : {-1ll, 90ll}) {
            JoinCase c;
            const int o[3] = {o0, o1, o2};
            for (int i = 0; i < 3; ++i) {
              c.rc[i] = OUTCOME_RC[o[i]];
              c.err[i] = (o[i] == O_BAD_IDX || o[i] == O_IDENT) ? e[i] : -1;
              c.lo[i] = lo[i];
            }
            c.eof = eof;
            fn(c);
          }
}
// the rule, restated: in cell order the first outcome that is no Source error ends the join; else the lowest non-canonical exponent, else
// the lowest identity, else the planned Eof
static CellJoin join_rule(const JoinCase& c) {
  for (int i = 0; i < 3; ++i) {
    const bool source = c.rc[i] == ZK_OK || c.rc[i] == ZK_ERR_UNEXPECTED_IDENTITY || (c.rc[i] == ZK_ERR_BAD_ARGS && c.err[i] >= 0);
    if (!source) return {c.rc[i] == ZK_ERR_BAD_ARGS ? ZK_ERR_BAD_ARGS : c.rc[i] < 0 ? c.rc[i] : ZK_ERR_DEVICE, -1};
  }
  for (int want : {ZK_ERR_BAD_ARGS, ZK_ERR_UNEXPECTED_IDENTITY}) {
    long long best = -1;
    for (int i = 0; i < 3; ++i)
      if (c.rc[i] == want && (best < 0 || c.err[i] + (long long)c.lo[i] < best)) best = c.err[i] + (long long)c.lo[i];
    if (best >= 0) return {want, best};
  }
  return c.eof >= 0 ? CellJoin{ZK_ERR_UNEXPECTED_EOF, c.eof} : CellJoin{ZK_OK, -1};
}
static void check_join() {
  for_join_cases([](const JoinCase& c) {
    const CellJoin got = join_of(c.rc, c.err, c.lo, 3, c.eof), want = join_rule(c);
    ++g_cases;
    CHECK(got.rc == want.rc && got.index == want.index, "rc=%d,%d,%d err=%lld,%lld,%lld eof=%lld: (%d, %lld) want (%d, %lld)", c.rc[0], c.rc[1], c.rc[2], c.err[0], c.err[1],
          c.err[2], c.eof, got.rc, got.index, want.rc, want.index);
  });
  const CellJoin none = join_of(nullptr, nullptr, nullptr, 0, 17);   // no cell at all (the Eof at the first exponent)
  ++g_cases;
  CHECK(none.rc == ZK_ERR_UNEXPECTED_EOF && none.index == 17, "no cells");
}

// ---------------------------------------------------------------- range_parts, weight_cuts, shared_shift
struct WeightCase {
  const char* name;
  std::vector<uint32_t> row_ptr;
};
static std::vector<WeightCase> weight_cases() {
  std::vector<WeightCase> out;
  auto from_lens = [&](const char* name, const std::vector<uint32_t>& lens) {
    WeightCase w{name, {0}};
    for (uint32_t l : lens) w.row_ptr.push_back(w.row_ptr.back() + l);
    out.push_back(w);
  };
  std::vector<uint32_t> even(1024, 3), first(1024, 1), last(1024, 1), holes(1024, 0), rnd(1000);
  first[0] = 100000;
  last[1023] = 100000;
  for (size_t i = 0; i < holes.size(); i += 7) holes[i] = 40;
  Rng r{1};
  for (auto& l : rnd) l = (uint32_t)(r.next() % 9);
  from_lens("even", even);
  from_lens("heavy_first", first);
  from_lens("heavy_last", last);
  from_lens("empty_rows", holes);
  from_lens("random", rnd);
  from_lens("three_rows", {5, 0, 2});     // parts > n_rows can only be asked for directly (range_parts gives 1)
  from_lens("no_terms", std::vector<uint32_t>(300, 0));
  return out;
}
static const size_t WEIGHT_DEVS[] = {1, 2, 3, 8};

static void check_small() {
  for (uint64_t K : {32ull, 1024ull, 128ull})
    for (size_t d : {1, 2, 3, 8}) {
      ++g_cases;
      CHECK(range_parts(K * d, d, K) == d, "K=%" PRIu64 " d=%zu at the threshold", K, d);
      CHECK(range_parts(K * d - 1, d, K) == (d > 1 ? d - 1 : 1), "K=%" PRIu64 " d=%zu below the threshold", K, d);
      CHECK(range_parts(0, d, K) == 1 && range_parts(K - 1, d, K) == 1 && range_parts(K << 20, d, K) == d, "K=%" PRIu64 " d=%zu ends", K, d);
    }
  for (const WeightCase& w : weight_cases()) {
    const size_t n_rows = w.row_ptr.size() - 1, nnz = w.row_ptr.back();
    for (size_t parts : {(size_t)1, (size_t)2, (size_t)3, (size_t)8, n_rows + 5}) {
      const std::vector<size_t> cut = weight_cuts(w.row_ptr.data(), n_rows, nnz, parts);
      ++g_cases;
      CHECK(cut.size() == parts + 1 && cut.front() == 0 && cut.back() == n_rows, "%s parts=%zu: ends", w.name, parts);
      for (size_t d = 0; d + 1 < cut.size(); ++d) CHECK(cut[d] <= cut[d + 1] && cut[d + 1] <= n_rows, "%s parts=%zu: cut %zu", w.name, parts, d);
      // part d starts at the first row r at which r rows and their terms reach d / parts of the weight (past the last row: never reached)
      const size_t weight = n_rows + nnz;
      auto reached = [&](size_t r, size_t d) { return r + w.row_ptr[r] >= weight * d / parts; };
      for (size_t d = 1; d < parts; ++d)
        CHECK((cut[d] == n_rows || reached(cut[d], d)) && (cut[d] == 0 || !reached(cut[d] - 1, d)), "%s parts=%zu: cut %zu = %zu is not where the weight is reached", w.name,
              parts, d, cut[d]);
    }
  }
  alignas(64) static char buf[64 * 64];
  const size_t rec = 64;
  const char* v1 = buf + 4 * rec;
  ++g_cases;
  for (size_t s : {0, 1, 16}) CHECK(shared_shift(v1, v1 + s * rec, rec, 20) == s, "shift %zu", s);
  CHECK(shared_shift(v1, v1 + 17 * rec, rec, 20) == (size_t)-1, "shift 17");
  CHECK(shared_shift(v1, v1 + 5 * rec, rec, 3) == (size_t)-1, "shift past n");
  CHECK(shared_shift(v1, v1 + 3 * rec, rec, 3) == 3, "shift == n");
  CHECK(shared_shift(v1, v1 + rec + 8, rec, 20) == (size_t)-1, "misaligned");
  CHECK(shared_shift(v1, v1 - rec, rec, 20) == (size_t)-1, "v2 < v1");
  CHECK(shared_shift(v1, nullptr, rec, 20) == (size_t)-1, "no v2");
  CHECK(shared_shift(v1, v1 + 2 * 128, 128, 20) == 2, "G2 records");
  ++g_cases;
  CHECK(msm_host_args_ok(buf, 1, buf, 1, buf) && msm_host_args_ok(nullptr, 0, nullptr, 0, buf), "good arguments");
  CHECK(!msm_host_args_ok(buf, 1, buf, 1, nullptr) && !msm_host_args_ok(nullptr, 1, buf, 1, buf) && !msm_host_args_ok(buf, 1, nullptr, 1, buf), "null pointers");
  CHECK(!msm_host_args_ok(buf, 1ull << 31, buf, 1, buf) && !msm_host_args_ok(buf, 1, buf, 1ull << 31, buf), "sizes past 2^31 - 1");
  // the knobs: parsing and clamping
  struct { const char* name; const char* value; bool (*ok)(const HostKnobs&); } knob_cases[] = {
      {nullptr, nullptr, [](const HostKnobs& K) { return K.chunk_growth == 1.8 && K.chunk_first_log == 0 && K.chunk_test == 0 && K.plan_p == 0 && K.plan_w == 0 && K.multi_min_log == 20 && K.dense_piece == (size_t)1 << 22; }},
      {"MI355ZK_HOST_CHUNK_GROWTH", "150", [](const HostKnobs& K) { return K.chunk_growth == 1.5; }},
      {"MI355ZK_HOST_CHUNK_GROWTH", "99", [](const HostKnobs& K) { return K.chunk_growth == 1.8; }},
      {"MI355ZK_HOST_CHUNK_FIRST", "22", [](const HostKnobs& K) { return K.chunk_first_log == 22; }},
      {"MI355ZK_HOST_CHUNK_FIRST", "15", [](const HostKnobs& K) { return K.chunk_first_log == 0; }},
      {"MI355ZK_HOST_CHUNK_FIRST", "31", [](const HostKnobs& K) { return K.chunk_first_log == 0; }},
      {"MI355ZK_HOST_CHUNK_TEST", "100", [](const HostKnobs& K) { return K.chunk_test == 96; }},
      {"MI355ZK_HOST_CHUNK_TEST", "31", [](const HostKnobs& K) { return K.chunk_test == 0; }},
      {"MI355ZK_MULTI_PLAN", "2x3", [](const HostKnobs& K) { return K.plan_p == 2 && K.plan_w == 3; }},
      {"MI355ZK_MULTI_PLAN", "0x1", [](const HostKnobs& K) { return K.plan_p == 0 && K.plan_w == 0; }},
      {"MI355ZK_MULTI_PLAN", "4", [](const HostKnobs& K) { return K.plan_p == 0 && K.plan_w == 0; }},
      {"MI355ZK_MULTI_MIN_LOG", "6", [](const HostKnobs& K) { return K.multi_min_log == 6; }},
      {"MI355ZK_MULTI_MIN_LOG", "-3", [](const HostKnobs& K) { return K.multi_min_log == 0; }},
      {"MI355ZK_MULTI_MIN_LOG", "40", [](const HostKnobs& K) { return K.multi_min_log == 30; }},
      {"MI355ZK_DENSE_PIECE_TEST", "100", [](const HostKnobs& K) { return K.dense_piece == 100; }},
      {"MI355ZK_DENSE_PIECE_TEST", "15", [](const HostKnobs& K) { return K.dense_piece == (size_t)1 << 22; }}};
  for (const auto& k : knob_cases) {
    set_knob(k.name, k.value);
    ++g_cases;
    CHECK(k.ok(host_knobs()), "knob %s=%s", k.name ? k.name : "(none)", k.value ? k.value : "");
  }
  set_knob(nullptr, nullptr);
}

// ---------------------------------------------------------------- dump
static void dump() {
  for (uint64_t n : CUT_N)
    for (int up = 0; up < 2; ++up) {
      std::printf("cuts n=%" PRIu64 " upload=%d:", n, up);
      for (uint64_t c : cuts_of(n, up != 0)) std::printf(" %" PRIu64, c);
      std::printf("\n");
    }
  for (uint64_t n : CELL_N)
    for (size_t devs : CELL_DEVS)
      for (int with_map = 0; with_map < 2; ++with_map) {
        const CellCase cc = cell_case(n, with_map != 0);
        const CellPlan C = cells_of(cc.P, CELL_BASE_OFFSET, devs);
        std::printf("cells n=%" PRIu64 " devs=%zu map=%d live=%" PRIu64 " eof=%lld: pg=%u wg=%u cut=", n, devs, with_map, cc.P.live(), cc.P.eof_index, C.pg, C.wg);
        for (size_t i = 0; i < C.cut.size(); ++i) std::printf("%s%" PRIu64, i ? "," : "", C.cut[i]);
        for (const HostCell& c : C.cells) std::printf(" [%u:%" PRIu64 "-%" PRIu64 "/%u@%" PRIu64 "+%" PRIu64 "]", c.slot, c.lo, c.hi, c.wgi, c.boff, c.used);
        std::printf("\n");
      }
  for_join_cases([](const JoinCase& c) {
    const CellJoin j = join_of(c.rc, c.err, c.lo, 3, c.eof);
    std::printf("join rc=%d,%d,%d err=%lld,%lld,%lld eof=%lld: rc=%d index=%lld\n", c.rc[0], c.rc[1], c.rc[2], c.err[0], c.err[1], c.err[2], c.eof, j.rc, j.index);
  });
  for (const WeightCase& w : weight_cases())
    for (size_t devs : WEIGHT_DEVS) {
      std::printf("weight %s devs=%zu:", w.name, devs);
      for (size_t c : wcuts_of(w.row_ptr.data(), w.row_ptr.size() - 1, w.row_ptr.back(), devs)) std::printf(" %zu", c);
      std::printf("\n");
    }
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "dump") {
    dump();
    return 0;
  }
  if (mode != "plan") {
    std::fprintf(stderr, "usage: test_host_plan plan | dump\n");
    return 2;
  }
  check_density();
  check_cuts();
  check_cells();
  check_join();
  check_small();
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("ok %ld\n", g_cases);
  return 0;
}
