// The batch inversion of csrc/fr_inverse.hpp as a whole process of its own: the lane routines, the product tree and the carry chunks in the
// kernels' grouping, on the host compiler alone (built plainly and with AddressSanitizer + UndefinedBehaviorSanitizer by
// tests/test_fr_inverse_san_host.py).  An inverse is unique, so the check is in[i] * out[i] == 1 for every non-zero input, out[i] == 0 for every
// zero, the count of zeros, and that nothing past n is written -- at the edge sizes of the grouping, in place and out of place, and with a zero in
// every position of one run and in every pair of positions of it.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../phase2-bn254_amd/csrc/fr_inverse.hpp"

using zk::Fr;

static int g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                       \
  do {                                         \
    ++g_checks;                                \
    if (!(cond)) {                             \
      ++g_failed;                              \
      std::fprintf(stderr, "FAILED %s: ", #cond); \
      std::fprintf(stderr, __VA_ARGS__);       \
      std::fprintf(stderr, "\n");              \
    }                                          \
  } while (0)

static uint64_t g_state = 0x9E3779B97F4A7C15ull;
static uint32_t next32() {   // splitmix64
  uint64_t z = (g_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return (uint32_t)((z ^ (z >> 31)) >> 16);
}
static Fr random_fr() {   // a canonical non-zero element: random limbs with the top one below r's, times R^2 (any canonical value will do)
  Fr a;
  for (int i = 0; i < 8; ++i) a.l[i] = next32();
  a.l[7] %= zk::FrParams::P[7];
  a.l[0] |= 1u;
  return zk::from_canonical(a);
}

static void run_case(const std::vector<Fr>& in, bool in_place, const char* what) {
  const size_t n = in.size(), guard = 3;
  Fr mark;
  for (int i = 0; i < 8; ++i) mark.l[i] = 0x5A5A5A5Au;
  std::vector<Fr> buf(n + guard, mark);
  if (in_place)
    for (size_t i = 0; i < n; ++i) buf[i] = in[i];
  uint32_t want_zeros = 0;
  for (const Fr& a : in) want_zeros += a.is_zero() ? 1 : 0;
  const uint32_t zeros = n ? zk::inv_batch_host(buf.data(), in_place ? buf.data() : in.data(), n) : 0;
  CHECK(zeros == want_zeros, "%s n=%zu: %u zeros counted, %u expected", what, n, zeros, want_zeros);
  const Fr one = Fr::one();
  size_t bad = 0;
  for (size_t i = 0; i < n; ++i) bad += in[i].is_zero() ? !buf[i].is_zero() : zk::mul(in[i], buf[i]) != one;
  CHECK(bad == 0, "%s n=%zu in_place=%d: %zu wrong elements", what, n, (int)in_place, bad);
  for (size_t i = n; i < n + guard; ++i) CHECK(buf[i] == mark, "%s n=%zu: element %zu past the end was written", what, n, i);
}

static std::vector<Fr> randoms(size_t n) {
  std::vector<Fr> a(n);
  for (Fr& x : a) x = random_fr();
  return a;
}

int main() {
  const size_t run = zk::INV_RUN, tile = zk::INV_TILE;
  const size_t sizes[] = {0, 1, 2, run - 1, run, run + 1, tile - 1, tile, tile + 1, 2 * tile + 3};
  for (size_t n : sizes)
    for (int in_place = 0; in_place < 2; ++in_place) {
      std::vector<Fr> a = randoms(n);
      run_case(a, in_place != 0, "random");
      if (n) {
        a[0] = Fr::zero();
        a[n - 1] = Fr::zero();
        a[n / 2] = Fr::zero();
        run_case(a, in_place != 0, "zeros at the ends and in the middle");
        run_case(std::vector<Fr>(n, Fr::zero()), in_place != 0, "all zero");
        run_case(std::vector<Fr>(n, Fr::one()), in_place != 0, "all one");
      }
    }
  // a zero in every position, and in every pair of positions, of the second run of a vector of three runs and one element
  const std::vector<Fr> base = randoms(3 * run + 1);
  for (size_t i = 0; i < run; ++i)
    for (size_t j = i; j < run; ++j) {
      std::vector<Fr> a = base;
      a[run + i] = Fr::zero();
      a[run + j] = Fr::zero();
      run_case(a, (i + j) % 2 == 1, "zeros in one run");
    }
  // (carry_width + 1) tiles and one element, every run product one but the last tile's: the second chunk of the carry
  {
    std::vector<Fr> a((size_t)(zk::INV_CARRY_W + 1) * tile + 1, Fr::one());
    for (size_t i = a.size() - 5; i < a.size(); ++i) a[i] = random_fr();
    a[7] = random_fr();
    a[tile] = Fr::zero();
    run_case(a, true, "two carry chunks");
  }
  if (g_failed) {
    std::printf("FAILED %d of %d\n", g_failed, g_checks);
    return 1;
  }
  std::printf("ok %d\n", g_checks);
  return 0;
}
