// A caller that keeps its bases the way bellman does -- `Arc<Vec<G1Affine>>` of `{ x: Fq, y: Fq, infinity: bool }` records (72 B;
// G2Affine 136 B, pairing/src/bn256/ec.rs:14-18) -- hands them to the library as they lie in memory through the strided entry points
// (include/mi355zk.h: mi355zk_bn254_g{1,2}_msm_strided, mi355zk_bases_cache_pin_strided), checked against the CPU oracle
// (TEST INFRASTRUCTURE: links oracle/_build/liboracle.so).  Built by tests/test_msm_strided_host.py, run by tests/test_gpu_msm_strided.py;
// prints "ok <name>" lines and exits 0 on success.
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <random>
#include <vector>

#include "../../include/mi355zk.h"

extern "C" {
void oracle_g1_mul_many_affine(uint64_t* out_affine, const uint64_t base_affine[8], const uint64_t* ks, size_t n);
void oracle_g2_mul_many_affine(uint64_t* out_affine, const uint64_t base_affine[16], const uint64_t* ks, size_t n);
int oracle_g1_multiexp(const uint64_t* bases, size_t n_bases, size_t base_offset, const uint64_t* scalars, size_t n_scalars,
                       const uint32_t* density, size_t density_bits, int threads, uint64_t out_xyz[12]);
int oracle_g2_multiexp(const uint64_t* bases, size_t n_bases, size_t base_offset, const uint64_t* scalars, size_t n_scalars,
                       const uint32_t* density, size_t density_bits, int threads, uint64_t out_xyz[24]);
void oracle_g1_to_affine(uint64_t r[8], const uint64_t p[12]);
void oracle_g2_to_affine(uint64_t r[16], const uint64_t p[24]);
}

// the Rust structs' layout: fields in order, bool after the coordinates, padded to the u64 alignment
struct G1AffineLike {
  uint64_t x[4], y[4];
  bool infinity;
};
struct G2AffineLike {
  uint64_t x[8], y[8];  // c0 || c1
  bool infinity;
};
static_assert(sizeof(G1AffineLike) == 72, "G1Affine is 72 bytes");
static_assert(sizeof(G2AffineLike) == 136, "G2Affine is 136 bytes");
static_assert(offsetof(G1AffineLike, x) == 0 && offsetof(G1AffineLike, y) == 32 && offsetof(G1AffineLike, infinity) == 64, "G1 offsets");
static_assert(offsetof(G2AffineLike, x) == 0 && offsetof(G2AffineLike, y) == 64 && offsetof(G2AffineLike, infinity) == 128, "G2 offsets");

static const uint64_t G1_GEN[8] = {0xd35d438dc58f0d9dULL, 0x0a78eb28f5c70b3dULL, 0x666ea36f7879462cULL, 0x0e0a77c19a07df2fULL,
                                   0xa6ba871b8b1e1b3aULL, 0x14f1d651eb8e167bULL, 0xccdd46def0f28c58ULL, 0x1c14ef83340fbe5eULL};
static const uint64_t G2_GEN[16] = {0x8e83b5d102bc2026ULL, 0xdceb1935497b0172ULL, 0xfbb8264797811adfULL, 0x19573841af96503bULL,
                                    0xafb4737da84c6140ULL, 0x6043dd5a5802d8c4ULL, 0x09e950fc52a02f86ULL, 0x14fef0833aea7b6bULL,
                                    0x619dfa9d886be9f6ULL, 0xfe7fd297f59e9b78ULL, 0xff9e1a62231b7dfeULL, 0x28fd7eebae9e4206ULL,
                                    0x64095b56c71856eeULL, 0xdc57f922327d3cbbULL, 0x55f935be33351076ULL, 0x0da4a0e693fd6482ULL};
static const uint64_t FQ_ONE[4] = {0xd35d438dc58f0d9dULL, 0x0a78eb28f5c70b3dULL, 0x666ea36f7879462cULL, 0x0e0a77c19a07df2fULL};  // R mod q

#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); return 1; } } while (0)

static std::vector<uint64_t> scalars(std::mt19937_64& g, size_t n) {  // < 2^253: canonical FrRepr
  std::vector<uint64_t> s(4 * n);
  for (size_t i = 0; i < n; ++i) {
    for (int k = 0; k < 4; ++k) s[4 * i + k] = g();
    s[4 * i + 3] &= (1ULL << 61) - 1;
  }
  return s;
}

// n records k_i * G in the Rust layout, every 7th one the identity as the reference encodes it (x = 0, y = R, infinity = true); padding 0xA5
template <class A, int LIMBS>
static std::shared_ptr<const std::vector<A>> make_points(std::mt19937_64& g, size_t n, std::vector<uint64_t>* packed) {
  std::vector<uint64_t> ks = scalars(g, n);
  packed->assign(2 * LIMBS * n, 0);
  if (LIMBS == 4) oracle_g1_mul_many_affine(packed->data(), G1_GEN, ks.data(), n);
  else oracle_g2_mul_many_affine(packed->data(), G2_GEN, ks.data(), n);
  auto v = std::make_shared<std::vector<A>>(n);
  std::memset((void*)v->data(), 0xA5, n * sizeof(A));
  for (size_t i = 0; i < n; ++i) {
    A& a = (*v)[i];
    a.infinity = i % 7 == 3;
    if (a.infinity) {
      std::memset(a.x, 0, sizeof a.x);
      std::memset(a.y, 0, sizeof a.y);
      std::memcpy(a.y, FQ_ONE, 32);
      std::memset(packed->data() + 2 * LIMBS * i, 0, 16 * LIMBS);  // the packed form of the identity: all zero
    } else {
      std::memcpy(a.x, packed->data() + 2 * LIMBS * i, 8 * LIMBS);
      std::memcpy(a.y, packed->data() + 2 * LIMBS * i + LIMBS, 8 * LIMBS);
    }
  }
  return v;
}

template <class A, int LIMBS>
static int run_group(std::mt19937_64& g, const char* name) {
  const size_t n = 3000;
  std::vector<uint64_t> packed;
  auto v = make_points<A, LIMBS>(g, n, &packed);
  std::vector<uint64_t> s = scalars(g, n);
  for (size_t i = 3; i < n; i += 7) std::memset(&s[4 * i], 0, 32);  // zero exponents under the identities
  uint64_t got[3 * 2 * LIMBS], want[3 * 2 * LIMBS], ga[2 * LIMBS], wa[2 * LIMBS];  // Jacobian X || Y || Z, affine x || y
  const int group = LIMBS == 4 ? 1 : 2;
  int rc = group == 1 ? mi355zk_bn254_g1_msm_strided(v->data(), n, sizeof(A), offsetof(A, x), offsetof(A, y), offsetof(A, infinity), 0, s.data(), n, nullptr, 0, got)
                      : mi355zk_bn254_g2_msm_strided(v->data(), n, sizeof(A), offsetof(A, x), offsetof(A, y), offsetof(A, infinity), 0, s.data(), n, nullptr, 0, got);
  CHECK(rc == 0);
  rc = group == 1 ? oracle_g1_multiexp(packed.data(), n, 0, s.data(), n, nullptr, 0, 4, want) : oracle_g2_multiexp(packed.data(), n, 0, s.data(), n, nullptr, 0, 4, want);
  CHECK(rc == 0);
  if (group == 1) { oracle_g1_to_affine(ga, got); oracle_g1_to_affine(wa, want); }
  else { oracle_g2_to_affine(ga, got); oracle_g2_to_affine(wa, want); }
  CHECK(std::memcmp(ga, wa, sizeof ga) == 0);
  std::printf("ok %s\n", name);
  return 0;
}

int main() {
  std::mt19937_64 g(0x5a17de);
  if (mi355zk_init(nullptr, 0) != 0) { std::puts("FAILED mi355zk_init"); return 1; }
  CHECK(mi355zk_abi_version() == MI355ZK_ABI_VERSION);
  if (run_group<G1AffineLike, 4>(g, "strided_g1_rust_layout")) return 1;
  if (run_group<G2AffineLike, 8>(g, "strided_g2_rust_layout")) return 1;

  {  // the CRS held as shared_ptr<const vector<G1Affine>> (the reference's Arc<Vec<G>>): pinned once, then only the exponents travel
    const size_t n = 5000;
    std::vector<uint64_t> packed;
    std::shared_ptr<const std::vector<G1AffineLike>> crs = make_points<G1AffineLike, 4>(g, n, &packed);
    std::vector<uint64_t> s = scalars(g, n);
    for (size_t i = 3; i < n; i += 7) std::memset(&s[4 * i], 0, 32);
    CHECK(mi355zk_bases_cache_pin_strided(crs->data(), n, sizeof(G1AffineLike), offsetof(G1AffineLike, x), offsetof(G1AffineLike, y),
                                          offsetof(G1AffineLike, infinity), 1, 0) == 0);
    uint64_t want[12], wa[8];
    CHECK(oracle_g1_multiexp(packed.data(), n, 0, s.data(), n, nullptr, 0, 4, want) == 0);
    oracle_g1_to_affine(wa, want);
    for (int k = 0; k < 2; ++k) {
      uint64_t got[12], ga[8];
      CHECK(mi355zk_bn254_g1_msm_strided(crs->data(), n, 72, 0, 32, 64, 0, s.data(), n, nullptr, 0, got) == 0);
      oracle_g1_to_affine(ga, got);
      CHECK(std::memcmp(ga, wa, 64) == 0);
    }
    size_t dbytes = 0, tbytes = 0;
    CHECK(mi355zk_bases_cache_info(crs->data(), &dbytes, &tbytes) == 1 && dbytes == n * 64);
    mi355zk_bases_cache_invalidate(crs->data());
    CHECK(mi355zk_bases_cache_info(crs->data(), &dbytes, &tbytes) == 0);
    std::puts("ok strided_pinned_shared_ptr");

    // a flagged base under a non-zero exponent: UnexpectedIdentity, named by its exponent index
    s[4 * 10] = 5;
    uint64_t got[12];
    CHECK(mi355zk_bn254_g1_msm_strided(crs->data(), n, 72, 0, 32, 64, 0, s.data(), n, nullptr, 0, got) == MI355ZK_ERR_UNEXPECTED_IDENTITY);
    CHECK(mi355zk_last_error_index() == 10);
    std::puts("ok strided_identity_error");
  }
  mi355zk_shutdown();
  return 0;
}
