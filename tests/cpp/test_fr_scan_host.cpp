// The prefix scans of csrc/fr_scan.hpp as a whole process of its own: the lane routines and the carry chunks in the kernels' grouping, on the
// host compiler alone (built plainly and with AddressSanitizer + UndefinedBehaviorSanitizer by tests/test_fr_scan_san_host.py).  The check is
// the recurrence itself, step by step: out[i] == out[i-1] o term[i] (inclusive) or out[i] == out[i-1] o term[i-1] (exclusive), the first
// element, the total, and that nothing past n is written -- at the edge sizes of the grouping, in place and out of place, products and sums,
// with and without the second operand, with a zero in every position of one run, and across two carry chunks.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../phase2-bn254_amd/csrc/fr_scan.hpp"

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
static Fr random_fr() {   // a canonical non-zero element
  Fr a;
  for (int i = 0; i < 8; ++i) a.l[i] = next32();
  a.l[7] %= zk::FrParams::P[7];
  a.l[0] |= 1u;
  return zk::from_canonical(a);
}
static std::vector<Fr> randoms(size_t n) {
  std::vector<Fr> a(n);
  for (Fr& x : a) x = random_fr();
  return a;
}

template <class Op>
static void run_case(const std::vector<Fr>& in, const std::vector<Fr>* num, bool exclusive, bool in_place, const char* what) {
  const size_t n = in.size(), guard = 3;
  Fr mark;
  for (int i = 0; i < 8; ++i) mark.l[i] = 0x5A5A5A5Au;
  std::vector<Fr> buf(n + guard, mark);
  if (in_place)
    for (size_t i = 0; i < n; ++i) buf[i] = in[i];
  // exactly n elements are handed over, so that the sanitizer sees a read past the end of either operand
  std::vector<Fr> src(in), nm(num ? *num : std::vector<Fr>());
  const Fr total = zk::scan_host<Op>(n ? buf.data() : nullptr, in_place ? buf.data() : src.data(), num ? nm.data() : nullptr, n, exclusive);
  size_t bad = 0;
  Fr acc = Op::identity();
  for (size_t i = 0; i < n; ++i) {   // out[i] from out[i-1], one step at a time
    const Fr term = num ? zk::mul((*num)[i], in[i]) : in[i];
    const Fr next = Op::op(acc, term);
    bad += buf[i] != (exclusive ? acc : next);
    acc = next;
  }
  CHECK(bad == 0, "%s n=%zu exclusive=%d in_place=%d num=%d: %zu wrong elements", what, n, (int)exclusive, (int)in_place, (int)(num != nullptr), bad);
  CHECK(total == acc, "%s n=%zu exclusive=%d: the total differs", what, n, (int)exclusive);
  for (size_t i = n; i < n + guard; ++i) CHECK(buf[i] == mark, "%s n=%zu: element %zu past the end was written", what, n, i);
}

static void run_all(const std::vector<Fr>& in, const std::vector<Fr>* num, bool in_place, const char* what) {
  for (int ex = 0; ex < 2; ++ex) {
    run_case<zk::ScanProduct>(in, num, ex != 0, in_place, what);
    run_case<zk::ScanSum>(in, num, ex != 0, in_place, what);
  }
}

int main() {
  const size_t run = zk::SCAN_RUN, tile = zk::SCAN_TILE;
  const size_t sizes[] = {0, 1, 2, run - 1, run, run + 1, tile - 1, tile, tile + 1, 2 * tile + 3};
  for (size_t n : sizes)
    for (int in_place = 0; in_place < 2; ++in_place) {
      const std::vector<Fr> a = randoms(n), num = randoms(n);
      run_all(a, nullptr, in_place != 0, "random");
      run_all(a, &num, in_place != 0, "random with a second operand");
      if (n) {
        run_all(std::vector<Fr>(n, Fr::one()), nullptr, in_place != 0, "all one");
        std::vector<Fr> z = a;
        z[n - 1] = Fr::zero();
        run_all(z, &num, in_place != 0, "zero last");
        z[n / 2] = Fr::zero();
        z[0] = Fr::zero();
        run_all(z, nullptr, in_place != 0, "zeros at the ends and in the middle");
      }
    }
  // a zero in every position of the second run of a vector of three runs and one element
  const std::vector<Fr> base = randoms(3 * run + 1), base_num = randoms(3 * run + 1);
  for (size_t i = 0; i < run; ++i) {
    std::vector<Fr> a = base;
    a[run + i] = Fr::zero();
    run_all(a, i % 2 ? &base_num : nullptr, i % 2 == 0, "a zero in one run");
    std::vector<Fr> m = base_num;   // ... and the same zero in the second operand
    m[run + i] = Fr::zero();
    run_all(base, &m, i % 2 == 1, "a zero in the second operand");
  }
  // (carry_width + 1) tiles and one element: the second chunk of the carry
  {
    std::vector<Fr> a((size_t)(zk::SCAN_CARRY_W + 1) * tile + 1, Fr::one());
    for (size_t i = 0; i < a.size(); i += 977) a[i] = random_fr();
    for (size_t i = a.size() - 5; i < a.size(); ++i) a[i] = random_fr();
    run_case<zk::ScanProduct>(a, nullptr, false, true, "two carry chunks");
    run_case<zk::ScanSum>(a, nullptr, true, false, "two carry chunks");
    a[(size_t)zk::SCAN_CARRY_W * tile + 1] = Fr::zero();   // in the last tile but one
    run_case<zk::ScanProduct>(a, nullptr, true, false, "two carry chunks, a zero in the second");
  }
  if (g_failed) {
    std::printf("FAILED %d of %d\n", g_failed, g_checks);
    return 1;
  }
  std::printf("ok %d\n", g_checks);
  return 0;
}
