// The batched multiexp's host arithmetic without a device (tests/test_msm_batch_host.py): the planner with MsmRequest::n_vectors, the
// pass split (msm_plan.hpp: msm_batch_split / msm_batch_pass) and the per-vector join (msm_join.hpp: msm_join_batch), compiled by the host
// compiler alone.
//   test_msm_batch_host plan          the grid n x B x group: invariants and limits of every pass plan, the refused requests; "ok <cases>" or FAIL lines
//   test_msm_batch_host join <file>   join cases from <file>; prints, per vector, what the join saw and what it returned, for the test to check with big ints
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../phase2-bn254_amd/csrc/curveu.hpp"
#include "../../phase2-bn254_amd/csrc/msm_join.hpp"
#include "../../phase2-bn254_amd/csrc/msm_plan.hpp"

using namespace zk;

static int g_fail = 0;
#define CHECK(cond)                                                                                                                   \
  do {                                                                                                                                \
    if (!(cond)) { ++g_fail; std::printf("FAIL %s (line %d): g=%d n=%" PRIu64 " B=%u per=%u\n", #cond, __LINE__, group, n, B, per); } \
  } while (0)

static std::vector<size_t> offsets(const MsmLayout& L) {
  return {L.keys, L.pairs, L.tile_hist, L.tile_off, L.csum, L.total, L.bin_start, L.out_start, L.gcnt, L.gcur, L.big_col, L.big_seg, L.big_plan, L.first,
          L.last, L.hist, L.sizes_b, L.ids_b, L.item_off, L.seg_sums, L.buckets, L.partA, L.partS, L.rc, L.wsums, L.err, L.sumtmp, L.total_bytes};
}

// every planned value of a single call, as text: B == 1 must give today's plan field by field
static std::string plan_text(const MsmPlan& P) {
  char buf[512];
  std::string s;
  std::snprintf(buf, sizeof buf, "rc=%d g=%d t=%d G=%u,%u,%u,%u,%u WD=%u w=%u..%u WL=%u nbk=%u m=%" PRIu64 " lv=%u tc=%" PRIu64 " f=%u,%u t2=%d,%u,%u,%u fb=%u rb=%u no=%u em=%u tr=%u,%" PRIu64,
                P.rc, P.group, (int)P.tmode, P.G.c, P.G.W, P.G.nb, P.G.rmul, P.G.rshift, P.WD, P.w_lo, P.w_hi, P.WL, P.n_buckets, P.m_max, P.n_levels,
                P.total_chunks, P.final_cnt, P.final_off, (int)P.tail2d, P.cols_log, P.t_cols, P.t_rows, P.final_bits, P.row_bits, P.n_out, P.e_max, P.tree_cnt,
                P.tree_tmp);
  s += buf;
  for (uint32_t w = 0; w < 64; ++w) { std::snprintf(buf, sizeof buf, " %u:%u", (unsigned)P.G.width[w], (unsigned)P.G.shift[w]); s += buf; }
  for (uint32_t k = 0; k <= MSM_MAX_LEVELS; ++k) { std::snprintf(buf, sizeof buf, " [%u,%u,%u]", P.lvl_cnt[k], P.lvl_chunks[k], P.lvl_logl[k]); s += buf; }
  for (uint32_t k = 0; k < MSM_MAX_JOBS; ++k) { std::snprintf(buf, sizeof buf, " e%u", P.e_k[k]); s += buf; }
  for (const ChunkPlan& C : P.chunks) {
    std::snprintf(buf, sizeof buf, " {%" PRIu64 ",%" PRIu64 ",%" PRIu64 ",%" PRIu64 " P=%u,%u,%u,%u,%u,%u nc=%u h=%u,%u,%u,%u ss=%d sp=%u,%u}", C.lo, C.n, C.m, C.np, C.P.lo_bits,
                  C.P.nbin, C.P.st, C.P.n_st, C.P.n_chunk, C.P.rows_per_chunk, C.ncell, C.heavy, C.heavy_seg, C.hb, C.max_items, (int)C.small_scan, C.split_t, C.split_hb);
    s += buf;
  }
  for (size_t o : offsets(P.L)) { std::snprintf(buf, sizeof buf, " %zu", o); s += buf; }
  return s;
}

static MsmPlan plan_of(int group, uint64_t n, uint32_t vectors, const MsmKnobs& K) {
  MsmRequest R;
  R.group = group; R.n = n; R.n_vectors = vectors;
  return msm_plan(R, K);
}

// the plan of one pass of `per` vectors: layout and every limit of the audit (msm_common.hpp: MSM_BATCH_*)
static void check_pass_plan(int group, uint64_t n, uint32_t B, uint32_t per, const MsmPlan& P, const MsmGeom& G1v) {
  CHECK(P.rc == ZK_OK);
  if (P.rc) return;
  const size_t rec = group == 1 ? sizeof(XYZZ<Fq>) : sizeof(XYZZ<Fq2>);
  const uint64_t WL = P.WL, nbk = P.n_buckets;
  // the geometry is that of ONE vector; the vectors multiply the bucket sets
  CHECK(std::memcmp(&P.G, &G1v, sizeof(MsmGeom)) == 0 && P.WD == G1v.W && P.w_lo == 0 && P.w_hi == P.WD && !P.tmode);
  CHECK(P.n_vectors == per && P.WL == per * P.WD && (uint64_t)P.n_buckets == WL * P.G.nb && P.m_max == n * WL && P.chunks.size() == 1);
  const ChunkPlan& C = P.chunks[0];
  CHECK(C.lo == 0 && C.n == n && C.np == n && C.m == n * WL && C.ncell == WL * C.P.nbin && C.P.st != 0);
  // the limits
  const uint64_t vals_cap = C.m + 3 * nbk + 4ull * C.ncell + 4;
  CHECK(WL <= MSM_BATCH_MAX_WINDOWS && per <= 65535u);                               // bucket sets per pass; the vector is a grid's y
  CHECK(nbk <= 0x7ffffff0ull && P.m_max <= 0xfffffff0ull && vals_cap <= 0xfffffff0ull);    // u32 bucket ids, pair positions, index lists
  CHECK((uint64_t)C.P.n_st * WL <= 0x7fffffffull && (uint64_t)C.ncell <= 0x7fffffffull);   // grids of the tile histogram / scatter and of the bucket pass
  CHECK(WL * C.P.nbin * 2 <= 2ull * PART_LDS_A && C.P.nbin <= 4 * PART_THREADS);           // choose_part's fits_lds
  CHECK((uint64_t)C.P.st * 8 + (uint64_t)C.P.nbin * 8 + 256 <= PART_LDS_MAX);
  for (uint32_t lv = 0; lv < P.n_levels; ++lv) CHECK((uint64_t)P.lvl_chunks[lv] * WL * 4 <= 0xffffffffull);   // a level's lanes, four per chunk at most
  const uint64_t sl = (P.tree_cnt + MSM_TREE_SLICE - 1) / MSM_TREE_SLICE;
  CHECK((uint64_t)(P.n_out + 2) * std::max<uint64_t>(sl, std::max(P.t_rows, P.t_cols)) * WL <= 0x7fffffffull);   // first_block[n_jobs] * WL
  CHECK(P.n_out + 2 <= MSM_MAX_JOBS && C.hb <= MSM_HEAVY_BLOCKS && C.hb <= nbk);
  CHECK(P.L.total_bytes <= MSM_BATCH_WS_MAX);
  CHECK(P.L.back_bytes() <= (uint64_t)MSM_BATCH_MAX_WINDOWS * MSM_MAX_JOBS * rec + 256 + 16);   // the pinned copy back
  // the layout: every region a multiple of 256, holding what the plan's own sizes ask for, none reaching into the next
  const uint64_t hb = C.hb, items = C.max_items, ncell = C.ncell;
  const std::vector<uint64_t> need = {vals_cap * 4, P.m_max * 8, (uint64_t)C.P.n_st * ((C.ncell + 1) & ~1u) * 2, (uint64_t)C.P.n_st * C.ncell * 4,
                                      (uint64_t)C.P.n_chunk * C.ncell * 4, ncell * 4, (ncell + 1) * 4, (ncell + 1) * 4, nbk * 4, nbk * 4, ncell * 4, ncell * 4,
                                      sizeof(BigPlan), (nbk + 1) * 4, (nbk + 1) * 4, MSM_SIZE_BINS * 4, nbk * 4, nbk * 4, (hb + 2) * 4, items * rec, nbk * rec,
                                      WL * P.total_chunks * rec, WL * P.total_chunks * rec, WL * (P.t_rows + P.t_cols) * rec, WL * P.n_out * rec, 16,
                                      WL * P.tree_tmp * 2 * rec};
  const std::vector<size_t> off = offsets(P.L);
  CHECK(off.size() == need.size() + 1 && off[0] == 0 && P.L.total_bytes % 256 == 0);
  for (size_t i = 0; i + 1 < off.size(); ++i) {
    CHECK(off[i] % 256 == 0 && off[i + 1] > off[i]);
    CHECK(off[i + 1] - off[i] >= need[i] && off[i + 1] - off[i] < need[i] + 256);
  }
  CHECK(P.L.back_bytes() == P.L.err + 16 - P.L.wsums && P.L.err >= P.L.wsums + WL * P.n_out * rec);
  // the schedule is per window, as in a single call
  uint32_t e = 0;
  for (uint32_t lv = 0; lv < P.n_levels; ++lv) { CHECK(P.e_k[lv] == e); e += P.lvl_logl[lv]; }
  for (uint32_t j = 0; j < P.final_bits; ++j) CHECK(P.e_k[P.n_levels + j] == e + j);
  for (uint32_t j = 0; j < P.row_bits; ++j) CHECK(P.e_k[P.n_levels + P.final_bits + j] == e + P.cols_log + j);
  CHECK(P.n_out == P.n_levels + P.final_bits + P.row_bits);
  (void)B;
}

static int run_plan() {
  const MsmKnobs K{};
  size_t cases = 0;
  bool several = false, whole = false, by_windows = false, by_bytes = false;
  for (int group = 1; group <= 2; ++group)
    for (uint64_t n : {(uint64_t)1, (uint64_t)33, (uint64_t)1 << 10, (uint64_t)20480, (uint64_t)1 << 16, (uint64_t)1 << 20})
      for (uint32_t B : {1u, 2u, 5u, 16u, 40u, 300u}) {
        ++cases;
        const MsmGeom G = choose_geom(n, group, 1, K);
        uint32_t per = msm_batch_split(n, B, G, group, K);
        CHECK(per >= 1 && per <= B);
        if (B == 1) {
          // today's plan, field by field: the request as every caller before the batch built it against the request with the new field spelled out
          MsmRequest R0;
          R0.group = group; R0.n = n;
          CHECK(per == 1 && plan_text(msm_plan(R0, K)) == plan_text(plan_of(group, n, 1, K)) && msm_plan(R0, K).rc == ZK_OK && msm_plan(R0, K).WL == G.W);
          continue;
        }
        // the passes cover 0 .. B exactly once, in order, each as large as the split says but the last
        const uint32_t n_pass = msm_batch_passes(B, per);
        std::vector<uint32_t> seen(B, 0);
        uint32_t next = 0;
        for (uint32_t p = 0; p < n_pass; ++p) {
          const MsmBatchPass pass = msm_batch_pass(B, per, p);
          CHECK(pass.first == next && pass.count >= 1 && pass.count <= per && (pass.count == per || p + 1 == n_pass));
          for (uint32_t v = 0; v < pass.count && pass.first + v < B; ++v) ++seen[pass.first + v];
          next = pass.first + pass.count;
          if (pass.count > 1) check_pass_plan(group, n, B, pass.count, plan_of(group, n, pass.count, K), G);
        }
        CHECK(next == B && msm_batch_pass(B, per, n_pass).count == 0);
        for (uint32_t v = 0; v < B; ++v) CHECK(seen[v] == 1);
        // ... and as large as the limits allow: one more vector is refused, or is past a budget
        if (per < B) {
          const MsmPlan Q = plan_of(group, n, per + 1, K);
          const bool windows = (uint64_t)(per + 1) * G.W > MSM_BATCH_MAX_WINDOWS;
          CHECK(Q.rc == ZK_ERR_BAD_ARGS || Q.L.total_bytes > MSM_BATCH_WS_MAX);
          CHECK(!windows || Q.rc == ZK_ERR_BAD_ARGS);
          by_windows |= windows;
          by_bytes |= Q.rc == ZK_OK;
          several = true;
        } else {
          whole = true;
        }
      }
  if (!(several && whole && by_windows && by_bytes)) { ++g_fail; std::printf("FAIL the grid misses a split: several=%d whole=%d windows=%d bytes=%d\n", several, whole, by_windows, by_bytes); }
  // the combinations a batch refuses (each accepted with one vector)
  const uint64_t n = 1u << 12, c2[3] = {0, 2048, n}, c1[2] = {0, n};
  struct { const char* what; MsmRequest R; } refused[6];
  for (auto& r : refused) r.R.n = n;
  refused[0].what = "table mode"; refused[0].R.table_stride = 4096; refused[0].R.table_c = 12;
  refused[1].what = "chunks"; refused[1].R.n_chunks = 2; refused[1].R.cuts = c2;
  refused[2].what = "a second base vector"; refused[2].R.two_sets = true;
  refused[3].what = "window groups"; refused[3].R.wgroups = 2;
  refused[4].what = "a streamed call of one chunk"; refused[4].R.cuts = c1;
  refused[5].what = "no vector";
  for (auto& r : refused) {
    ++cases;
    if (msm_plan(r.R, K).rc != ZK_OK) { ++g_fail; std::printf("FAIL '%s' is refused with one vector\n", r.what); }
    r.R.n_vectors = std::strcmp(r.what, "no vector") ? 3 : 0;
    if (msm_plan(r.R, K).rc != ZK_ERR_BAD_ARGS) { ++g_fail; std::printf("FAIL a batch with %s is not refused\n", r.what); }
  }
  {  // more bucket sets than a pass holds
    ++cases;
    const MsmGeom G = choose_geom(64, 1, 1, K);
    if (plan_of(1, 64, MSM_BATCH_MAX_WINDOWS / G.W, K).rc != ZK_OK || plan_of(1, 64, MSM_BATCH_MAX_WINDOWS / G.W + 1, K).rc != ZK_ERR_BAD_ARGS) {
      ++g_fail;
      std::printf("FAIL MSM_BATCH_MAX_WINDOWS is not the planner's bound\n");
    }
  }
  if (g_fail) return 1;
  std::printf("ok %zu\n", cases);
  return 0;
}

// ---------------------------------------------------------------- the join (the record helpers of tests/cpp/test_msm_host.cpp)
template <class F> struct Rec;
template <> struct Rec<Fq> {
  static XYZZ<Fq> of(const Affine<Fq>& a, const Affine<Fq>& b, bool two) {
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

struct JoinCase { int id, group; uint64_t n; uint32_t B; int serial; uint64_t seed; };

// one pass of B vectors: B * WD * n_out window sums s * G, joined per vector over ITS slice; one output line per vector
template <class F>
static void run_join_case(const JoinCase& jc, const Affine<F>& gen) {
  const MsmKnobs K{};
  const MsmPlan P = plan_of(jc.group, jc.n, jc.B, K);
  if (P.rc) { std::printf("case %d v=0 rc=%d\n", jc.id, P.rc); return; }
  const size_t per = (size_t)P.WD * P.n_out;
  std::vector<XYZZ<F>> h((size_t)P.WL * P.n_out);
  std::vector<uint64_t> sv(h.size());
  uint64_t x = jc.seed * 0x9e3779b97f4a7c15ull + 1;
  auto next = [&] { x ^= x << 13; x ^= x >> 7; x ^= x << 17; return x; };
  for (size_t i = 0; i < h.size(); ++i) {
    uint64_t s = next();
    if (next() % 5 == 0) s = 0;
    if (next() % 7 == 0) s &= 0xff;
    sv[i] = s;
    if (s == 0) { h[i] = XYZZ<F>::zero(); continue; }
    const uint64_t a = s - s / 2, b = s / 2;  // the record of a*G + b*G: ZZ and ZZZ are not 1
    h[i] = Rec<F>::of(mul_u64(gen, a), b ? mul_u64(gen, b) : gen, b != 0);
  }
  std::vector<Jacobian<F>> r(jc.B);
  bool parallel = false;
  msm_join_batch<F>(P, h.data(), jc.B, jc.serial != 0, r.data(), &parallel);
  for (uint32_t v = 0; v < jc.B; ++v) {
    std::printf("case %d v=%u rc=0 rmul=%u rshift=%u WD=%u WL=%u n_out=%u parallel=%d shift=", jc.id, v, P.G.rmul, P.G.rshift, P.WD, P.WL, P.n_out, (int)parallel);
    for (uint32_t w = 0; w < P.G.W; ++w) std::printf("%s%u", w ? "," : "", (unsigned)P.G.shift[w]);
    std::printf(" e_k=");
    for (uint32_t k = 0; k < P.n_out; ++k) std::printf("%s%u", k ? "," : "", P.e_k[k]);
    std::printf(" s=");
    for (size_t i = 0; i < per; ++i) std::printf("%s%" PRIu64, i ? "," : "", sv[v * per + i]);
    std::printf(" result=");
    if (r[v].is_zero()) { std::printf(" inf\n"); continue; }
    const F zi = inv(r[v].z), zi2 = sqr(zi);
    print_coord(mul(r[v].x, zi2));
    print_coord(mul(r[v].y, mul(zi2, zi)));
    std::printf("\n");
  }
}

static int run_join(const char* path) {
  FILE* f = std::fopen(path, "r");
  if (!f) { std::perror(path); return 2; }
  char a[80], b[80], c[80], d[80];
  if (std::fscanf(f, " g1 %79s %79s", a, b) != 2) return 2;
  const Affine<Fq> g1{fq_from_hex(a), fq_from_hex(b)};
  if (std::fscanf(f, " g2 %79s %79s %79s %79s", a, b, c, d) != 4) return 2;
  const Affine<Fq2> g2{Fq2{fq_from_hex(a), fq_from_hex(b)}, Fq2{fq_from_hex(c), fq_from_hex(d)}};
  JoinCase jc;
  while (std::fscanf(f, " case %d %d %" SCNu64 " %u %d %" SCNu64, &jc.id, &jc.group, &jc.n, &jc.B, &jc.serial, &jc.seed) == 6) {
    if (jc.group == 1) run_join_case<Fq>(jc, g1);
    else run_join_case<Fq2>(jc, g2);
  }
  std::fclose(f);
  return 0;
}

int main(int argc, char** argv) {
  const std::string mode = argc > 1 ? argv[1] : "";
  if (mode == "plan") return run_plan();
  if (mode == "join" && argc > 2) return run_join(argv[2]);
  std::fprintf(stderr, "usage: test_msm_batch_host plan | join <cases file>\n");
  return 2;
}
