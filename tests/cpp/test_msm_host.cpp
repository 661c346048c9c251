// The multiexp's host arithmetic without a device (tests/test_msm_join_host.py): the planner (msm_plan.hpp) and the window join
// (msm_join.hpp), compiled by the host compiler alone.
//   test_msm_host plan          invariants of every plan of the grid + one case per argument error; prints "ok <cases>" or FAIL lines
//   test_msm_host dump          every planned value of the grid, one line per case (knobs from the environment, as the library reads them)
//   test_msm_host join <file>   join cases from <file>; prints what the join saw and what it returned, for the test to check with big ints
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

#include "../../phase2-bn254_amd/csrc/curveu.hpp"
#include "../../phase2-bn254_amd/csrc/msm_join.hpp"
#include "../../phase2-bn254_amd/csrc/msm_plan.hpp"

using namespace zk;

// ---------------------------------------------------------------- the grid of plans
// the sizes of tests/test_msm_digits_host.py (SIZES): power-of-two windows and mixed-radix windows of several multipliers
static const struct { uint64_t n; uint32_t wgroups; } SIZES[] = {
    {1u << 10, 1}, {1u << 16, 1}, {1u << 20, 1}, {1u << 22, 2}, {1u << 24, 4}, {1u << 26, 4}, {1u << 26, 2}, {1u << 27, 4}, {1u << 28, 1},
    {20480, 1}, {98304, 1}, {40960, 2}, {14336, 1}, {12582912, 1}, {256, 4}, {8388608, 1}};

struct Case {
  std::string label;
  MsmRequest R;
  std::vector<uint64_t> cuts;  // (R.cuts points here once the case is in place)
};

static std::vector<Case> grid() {
  std::vector<Case> out;
  auto push = [&](const std::string& label, const MsmRequest& R, std::vector<uint64_t> cuts = {}) {
    out.push_back(Case{label, R, std::move(cuts)});
  };
  for (int group = 1; group <= 2; ++group) {
    for (const auto& s : SIZES)
      for (uint32_t wg = 0; wg < s.wgroups; wg += s.wgroups > 1 ? s.wgroups - 1 : 1) {  // the first and the last window group
        MsmRequest R;
        R.group = group; R.n = s.n; R.wgroups = s.wgroups; R.wgroup = wg;
        push("plain", R);
      }
    // streamed calls: 1, 2 and 5 chunks, inner cuts multiples of 32
    for (uint64_t n : {(uint64_t)1 << 16, (uint64_t)20480, (uint64_t)1 << 22, (uint64_t)1 << 26, (uint64_t)100000})
      for (uint32_t k : {1u, 2u, 5u}) {
        MsmRequest R;
        R.group = group; R.n = n; R.n_chunks = k;
        std::vector<uint64_t> cuts(k + 1);
        for (uint32_t i = 0; i <= k; ++i) cuts[i] = i == k ? n : (n * i / k) & ~31ull;
        push("chunks", R, cuts);
      }
    // table mode (ONE bucket set); 2^20 takes the 2-D tail on G1
    for (auto t : {std::pair<uint64_t, uint32_t>{1u << 16, 17}, {1u << 20, 20}, {1u << 20, 17}, {1u << 12, 8}}) {
      MsmRequest R;
      R.group = group; R.n = t.first; R.table_stride = t.first; R.table_c = t.second;
      push("table", R);
    }
    MsmRequest R2;  // a second base vector
    R2.group = group; R2.n = 1u << 14; R2.two_sets = true;
    push("two_sets", R2);
  }
  for (Case& c : out) c.R.cuts = c.cuts.empty() ? nullptr : c.cuts.data();
  return out;
}

static std::vector<size_t> offsets(const MsmLayout& L) {
  return {L.keys, L.pairs, L.tile_hist, L.tile_off, L.csum, L.total, L.bin_start, L.out_start, L.gcnt, L.gcur, L.big_col, L.big_seg, L.big_plan, L.first,
          L.last, L.hist, L.sizes_b, L.ids_b, L.item_off, L.seg_sums, L.buckets, L.partA, L.partS, L.rc, L.wsums, L.err, L.sumtmp, L.total_bytes};
}

static void dump(const Case& c, const MsmPlan& P) {
  const MsmRequest& R = c.R;
  std::printf("%s g=%d n=%" PRIu64 " wg=%u/%u chunks=%u two=%d table=%" PRIu64 ",%u: rc=%d", c.label.c_str(), R.group, R.n, R.wgroup, R.wgroups, R.n_chunks,
              (int)R.two_sets, R.table_stride, R.table_c, P.rc);
  if (P.rc) { std::printf("\n"); return; }
  std::printf(" G=%u,%u,%u,%u,%u WD=%u WL=%u w=%u..%u nbk=%u m_max=%" PRIu64 " levels=%u", P.G.c, P.G.W, P.G.nb, P.G.rmul, P.G.rshift, P.WD, P.WL, P.w_lo, P.w_hi,
              P.n_buckets, P.m_max, P.n_levels);
  for (uint32_t lv = 0; lv < P.n_levels; ++lv) std::printf(" [%u,%u,%u]", P.lvl_cnt[lv], P.lvl_chunks[lv], P.lvl_logl[lv]);
  std::printf(" total_chunks=%" PRIu64 " final=%u off=%u tail=%d rows=%u cols=%u fbits=%u rbits=%u clog=%u n_out=%u e_k=", P.total_chunks, P.final_cnt, P.final_off,
              (int)P.tail2d, P.t_rows, P.t_cols, P.final_bits, P.row_bits, P.cols_log, P.n_out);
  for (uint32_t k = 0; k < P.n_out; ++k) std::printf("%s%u", k ? "," : "", P.e_k[k]);
  std::printf(" tree=%u,%" PRIu64, P.tree_cnt, P.tree_tmp);
  for (const ChunkPlan& C : P.chunks)
    std::printf(" {%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 " P=%u,%u,%u,%u,%u,%u ncell=%u heavy=%u,%u,%u,%u small=%d split=%u,%u}", C.lo, C.n, C.m, C.np, C.P.lo_bits,
                C.P.nbin, C.P.st, C.P.n_st, C.P.n_chunk, C.P.rows_per_chunk, C.ncell, C.heavy, C.heavy_seg, C.hb, C.max_items, (int)C.small_scan, C.split_t, C.split_hb);
  std::printf(" L=");
  for (size_t o : offsets(P.L)) std::printf("%zu,", o);
  std::printf("\n");
}

// ---------------------------------------------------------------- plan invariants
static int g_fail = 0;
#define CHECK(cond, c)                                                                    \
  do {                                                                                    \
    if (!(cond)) { ++g_fail; std::printf("FAIL %s (line %d): ", #cond, __LINE__); dump(c, P); } \
  } while (0)

static void check_plan(const Case& c, const MsmPlan& P) {
  CHECK(P.rc == ZK_OK, c);
  if (P.rc) return;
  const size_t rec = c.R.group == 1 ? sizeof(XYZZ<Fq>) : sizeof(XYZZ<Fq2>);
  const MsmLayout& L = P.L;
  const uint64_t nbk = P.n_buckets, WL = P.WL;
  // what every region must hold, from the plan's own sizes
  uint64_t vals_cap = 0, tile_hist = 0, tile_off = 0, csum = 0, ncell = 0, hb = 0, items = 0;
  for (const ChunkPlan& C : P.chunks) {
    const uint64_t vc = C.m + 3 * nbk + 4ull * C.ncell + 4;
    CHECK(vc <= 0xfffffff0ull && C.m <= P.m_max && C.P.st != 0 && C.ncell == WL * C.P.nbin, c);
    vals_cap = std::max(vals_cap, vc);
    tile_hist = std::max<uint64_t>(tile_hist, (uint64_t)C.P.n_st * ((C.ncell + 1) & ~1u) * 2);
    tile_off = std::max<uint64_t>(tile_off, (uint64_t)C.P.n_st * C.ncell * 4);
    csum = std::max<uint64_t>(csum, (uint64_t)C.P.n_chunk * C.ncell * 4);
    ncell = std::max<uint64_t>(ncell, C.ncell);
    hb = std::max<uint64_t>(hb, C.hb);
    items = std::max<uint64_t>(items, C.max_items);
  }
  CHECK(P.m_max <= 0xfffffff0ull && P.n_out + 2 <= MSM_MAX_JOBS && P.n_out == P.n_levels + P.final_bits + P.row_bits, c);
  const std::vector<uint64_t> need = {vals_cap * 4, P.m_max * 8, tile_hist, tile_off, csum, ncell * 4, (ncell + 1) * 4, (ncell + 1) * 4, nbk * 4, nbk * 4, ncell * 4,
                                      ncell * 4, sizeof(BigPlan), (nbk + 1) * 4, (nbk + 1) * 4, MSM_SIZE_BINS * 4, nbk * 4, nbk * 4, (hb + 2) * 4, items * rec,
                                      nbk * rec, WL * P.total_chunks * rec, WL * P.total_chunks * rec, WL * (P.t_rows + P.t_cols) * rec, WL * P.n_out * rec, 16,
                                      WL * P.tree_tmp * 2 * rec};
  const std::vector<size_t> off = offsets(L);
  CHECK(off.size() == need.size() + 1 && off[0] == 0, c);
  for (size_t i = 0; i + 1 < off.size(); ++i) {
    CHECK(off[i] % 256 == 0 && off[i + 1] > off[i], c);       // aligned, strictly increasing
    CHECK(off[i + 1] - off[i] >= need[i], c);                 // no region reaches into the next
    CHECK(off[i + 1] - off[i] < need[i] + 256, c);            // ... and none is padded beyond its alignment
  }
  CHECK(L.total_bytes % 256 == 0, c);
  // gcnt and gcur are cleared by ONE memset of big_col - gcnt bytes
  CHECK(L.gcur == L.gcnt + align_up(nbk * 4) && L.big_col - L.gcnt == 2 * align_up(nbk * 4), c);
  // the copy back starts at wsums and ends with the 16 bytes of the error words
  CHECK(L.back_bytes() == L.err + 16 - L.wsums && L.err >= L.wsums + WL * P.n_out * rec && L.sumtmp >= L.err + 16, c);
  // the exponents of the partial sums
  uint32_t e = 0, e_max = 0;
  for (uint32_t lv = 0; lv < P.n_levels; ++lv) { CHECK(P.e_k[lv] == e, c); e += P.lvl_logl[lv]; }
  for (uint32_t j = 0; j < P.final_bits; ++j) CHECK(P.e_k[P.n_levels + j] == e + j, c);
  for (uint32_t j = 0; j < P.row_bits; ++j) CHECK(P.e_k[P.n_levels + P.final_bits + j] == e + P.cols_log + j, c);
  for (uint32_t k = 0; k < P.n_out; ++k) e_max = std::max(e_max, P.e_k[k]);
  CHECK(P.e_max == e_max && P.final_off == (P.n_levels == 0 ? 1u : 0u) && (P.row_bits == 0 || P.tail2d), c);
  CHECK(P.WD * c.R.wgroups == P.G.W && P.w_hi - P.w_lo == P.WD && P.WL == (P.tmode ? 1u : P.WD) && P.n_buckets == P.WL * P.G.nb, c);
}

static int run_plan() {
  const MsmKnobs K{};
  size_t cases = 0;
  bool tail = false, no_tail = false, no_levels = false;
  for (const Case& c : grid()) {
    const MsmPlan P = msm_plan(c.R, K);
    check_plan(c, P);
    tail |= P.row_bits > 0;
    no_tail |= !P.tail2d;
    no_levels |= P.n_levels == 0;
    ++cases;
  }
  if (!(tail && no_tail && no_levels)) { ++g_fail; std::printf("FAIL the grid misses a schedule: tail=%d no_tail=%d no_levels=%d\n", tail, no_tail, no_levels); }
  // every argument check of msm_device's planning, one case each (each must be refused; the request before the change must pass)
  const uint64_t n = 1u << 12;
  const uint64_t c2[3] = {0, 2048, n}, bad0[3] = {32, 2048, n}, badn[3] = {0, 2048, n - 32}, flat[3] = {0, 0, n}, odd[3] = {0, 2000, n};
  using Edit = std::function<void(MsmRequest&)>;
  const std::pair<const char*, Edit> errors[] = {
      {"wgroups == 0", [](MsmRequest& R) { R.wgroups = 0; }},
      {"wgroup >= wgroups", [](MsmRequest& R) { R.wgroups = 2; R.wgroup = 2; }},
      {"table: window groups", [](MsmRequest& R) { R.table_stride = 4096; R.table_c = 12; R.wgroups = 2; }},
      {"table: chunks", [&](MsmRequest& R) { R.table_stride = 4096; R.table_c = 12; R.n_chunks = 2; R.cuts = c2; }},
      {"table: second base vector", [](MsmRequest& R) { R.table_stride = 4096; R.table_c = 12; R.two_sets = true; }},
      {"table: c < 4", [](MsmRequest& R) { R.table_stride = 4096; R.table_c = 3; }},
      {"table: c > 24", [](MsmRequest& R) { R.table_stride = 4096; R.table_c = 25; }},
      {"table: base_offset > stride", [](MsmRequest& R) { R.table_stride = 4096; R.table_c = 12; R.base_offset = 4097; }},
      {"no chunk", [&](MsmRequest& R) { R.n_chunks = 0; R.cuts = c2; }},
      {"chunks without cuts (the planner's own check: msm_device cannot ask for it)", [](MsmRequest& R) { R.n_chunks = 2; }},
      {"cuts[0] != 0", [&](MsmRequest& R) { R.n_chunks = 2; R.cuts = bad0; }},
      {"cuts[last] != n", [&](MsmRequest& R) { R.n_chunks = 2; R.cuts = badn; }},
      {"chunks and a second base vector", [&](MsmRequest& R) { R.n_chunks = 2; R.cuts = c2; R.two_sets = true; }},
      {"empty chunk", [&](MsmRequest& R) { R.n_chunks = 2; R.cuts = flat; }},
      {"inner cut not a multiple of 32", [&](MsmRequest& R) { R.n_chunks = 2; R.cuts = odd; }},
      {"no window count divides into the groups", [](MsmRequest& R) { R.wgroups = 67; R.wgroup = 1; }},
      {"table: index past 31 bits", [](MsmRequest& R) { R.table_stride = 1u << 28; R.table_c = 17; }},
      {"pair positions past 32 bits", [](MsmRequest& R) { R.n = 0x7fffffffull; }},
      {"index lists past 32 bits", [](MsmRequest& R) { R.n = 390451568ull; R.table_stride = 1u << 20; R.table_c = 24; }},
  };
  // (the two remaining returns cannot be reached from any request: choose_part always finds a super-tile -- nbin <= 4096 -- and
  // n_out <= 8 levels + 24 bits leaves n_out + 2 <= MSM_MAX_JOBS)
  for (const auto& e : errors) {
    MsmRequest R;
    R.n = n;
    if (msm_plan(R, K).rc != ZK_OK) { ++g_fail; std::printf("FAIL the base request of '%s' is refused\n", e.first); }
    e.second(R);
    if (msm_plan(R, K).rc != ZK_ERR_BAD_ARGS) { ++g_fail; std::printf("FAIL '%s' is not refused\n", e.first); }
    ++cases;
  }
  {  // the streamed form of the base request, as the error cases cut it, is itself accepted
    MsmRequest R;
    R.n = n; R.n_chunks = 2; R.cuts = c2;
    if (msm_plan(R, K).rc != ZK_OK) { ++g_fail; std::printf("FAIL the two-chunk base request is refused\n"); }
  }
  if (g_fail) return 1;
  std::printf("ok %zu\n", cases);
  return 0;
}

// ---------------------------------------------------------------- the join
template <class F> struct Rec;
template <> struct Rec<Fq> {
  static XYZZ<Fq> of(const Affine<Fq>& a, const Affine<Fq>& b, bool two) {  // the record of a (+ b), as the accumulation leaves it
    XYZZU<FqParams> acc = XYZZU<FqParams>::zero();
    xyzzu_add_mixed(acc, a.x, a.y, false);
    if (two) xyzzu_add_mixed(acc, b.x, b.y, false);
    return xyzzu_to_r(acc);
  }
};
template <> struct Rec<Fq2> {
  static XYZZ<Fq2> of(const Affine<Fq2>& a, const Affine<Fq2>& b, bool two) {
    XYZZU2 acc = XYZZU2::zero();
    xyzzu2_add_mixed(acc, a.x, a.y, false);
    if (two) xyzzu2_add_mixed(acc, b.x, b.y, false);
    return xyzzu_to_r(acc);
  }
};

template <class F>
static Affine<F> mul_u64(const Affine<F>& g, uint64_t s) {  // s > 0
  XYZZ<F> acc = XYZZ<F>::zero();
  for (int b = 63; b >= 0; --b) {
    acc = xyzz_double(acc);
    if ((s >> b) & 1) xyzz_add_mixed(acc, g.x, g.y, false);
  }
  return xyzz_to_affine(acc);
}

static Fq fq_from_hex(const char* h) {
  Fq c = Fq::zero();
  const size_t len = std::strlen(h);
  for (size_t i = 0; i < len; ++i) {
    const char ch = h[len - 1 - i];
    const uint32_t d = ch <= '9' ? ch - '0' : (ch | 32) - 'a' + 10;
    if (i / 8 < 8) c.l[i / 8] |= d << (4 * (i % 8));
  }
  return from_canonical(c);
}
static void print_fq(const Fq& a) {
  const Fq c = to_canonical(a);
  std::printf(" ");
  for (int i = 7; i >= 0; --i) std::printf("%08x", c.l[i]);
}
static void print_coord(const Fq& a) { print_fq(a); }
static void print_coord(const Fq2& a) { print_fq(a.c0); print_fq(a.c1); }

struct JoinCase { int id, group; uint64_t n; uint32_t wgroups, wgroup, table_c; int serial; uint32_t final_max; int no_tail2d; uint64_t seed; };

template <class F>
static void run_join_case(const JoinCase& jc, const Affine<F>& gen) {
  MsmKnobs K{};
  if (jc.final_max) K.final_max = jc.final_max;
  K.no_tail2d = jc.no_tail2d != 0;
  MsmRequest R;
  R.group = jc.group; R.n = jc.n; R.wgroups = jc.wgroups; R.wgroup = jc.wgroup;
  if (jc.table_c) R.table_stride = jc.n, R.table_c = jc.table_c;
  const MsmPlan P = msm_plan(R, K);
  std::printf("case %d rc=%d", jc.id, P.rc);
  if (P.rc) { std::printf("\n"); return; }
  std::printf(" tmode=%d rmul=%u rshift=%u w_lo=%u WL=%u n_out=%u n_levels=%u row_bits=%u final_off=%u shift=", (int)P.tmode, P.G.rmul, P.G.rshift, P.w_lo, P.WL,
              P.n_out, P.n_levels, P.row_bits, P.final_off);
  for (uint32_t w = 0; w < P.G.W; ++w) std::printf("%s%u", w ? "," : "", (unsigned)P.G.shift[w]);
  std::printf(" e_k=");
  for (uint32_t k = 0; k < P.n_out; ++k) std::printf("%s%u", k ? "," : "", P.e_k[k]);
  // h_wsums[wl][k] = s * G as a record of the R domain; one entry in five is the zero record
  std::vector<XYZZ<F>> h((size_t)P.WL * P.n_out);
  uint64_t x = jc.seed * 0x9e3779b97f4a7c15ull + 1;
  auto next = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  std::printf(" s=");
  for (size_t i = 0; i < h.size(); ++i) {
    uint64_t s = next();
    if (next() % 5 == 0) s = 0;
    if (next() % 7 == 0) s &= 0xff;   // (small multiples: equal and opposite terms meet in the join's additions)
    std::printf("%s%" PRIu64, i ? "," : "", s);
    if (s == 0) { h[i] = XYZZ<F>::zero(); continue; }
    const uint64_t a = s - s / 2, b = s / 2;  // the record of a*G + b*G: ZZ and ZZZ are not 1
    h[i] = Rec<F>::of(mul_u64(gen, a), b ? mul_u64(gen, b) : gen, b != 0);
  }
  Jacobian<F> r;
  bool parallel = false;
  msm_join<F>(P, h.data(), jc.serial != 0, &r, &parallel);
  std::printf(" parallel=%d result=", (int)parallel);
  if (r.is_zero()) {
    std::printf(" inf\n");
    return;
  }
  const F zi = inv(r.z), zi2 = sqr(zi);
  print_coord(mul(r.x, zi2));
  print_coord(mul(r.y, mul(zi2, zi)));
  std::printf("\n");
}

static int run_join(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) { std::perror(path); return 2; }
  char a[80], b[80], c[80], d[80];
  Affine<Fq> g1{};
  Affine<Fq2> g2{};
  if (std::fscanf(f, " g1 %79s %79s", a, b) != 2) return 2;
  g1 = Affine<Fq>{fq_from_hex(a), fq_from_hex(b)};
  if (std::fscanf(f, " g2 %79s %79s %79s %79s", a, b, c, d) != 4) return 2;
  g2 = Affine<Fq2>{Fq2{fq_from_hex(a), fq_from_hex(b)}, Fq2{fq_from_hex(c), fq_from_hex(d)}};
  JoinCase jc;
  while (std::fscanf(f, " case %d %d %" SCNu64 " %u %u %u %d %u %d %" SCNu64, &jc.id, &jc.group, &jc.n, &jc.wgroups, &jc.wgroup, &jc.table_c, &jc.serial,
                     &jc.final_max, &jc.no_tail2d, &jc.seed) == 10) {
    if (jc.group == 1) run_join_case<Fq>(jc, g1);
    else run_join_case<Fq2>(jc, g2);
  }
  std::fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "plan") return run_plan();
  if (mode == "dump") {
    const MsmKnobs K = msm_knobs();
    for (const Case& c : grid()) dump(c, msm_plan(c.R, K));
    return 0;
  }
  if (mode == "join" && argc > 2) return run_join(argv[2]);
  std::fprintf(stderr, "usage: test_msm_host plan | dump | join <cases file>\n");
  return 2;
}
