// xyzzu_add_mixed, xyzzr_add and xyzzu_to_r (csrc/curveu.hpp) compiled for the HOST on the product's types (uint32_t limbs), as a stand-alone
// program: tests/test_mixed_add_trim_host.py builds it with -fsanitize=undefined,address and feeds it the cases of tests/mixed_add_trim_vectors.py.
//   stdin : one case per line, hexadecimal words:
//             0 n  acc[36]  n x (x[8] y[8] negate)    acc, then n mixed additions in a row            (acc: X, Y, ZZ, ZZZ on nine limbs each)
//             1    acc[36]  o[36]                     xyzzr_add(acc, o), both in register form
//   stdout: one line per case, 68 words: the accumulator afterwards, then its record (op 0: xyzzu_to_r, op 1: xyzzr_store)
// Nothing but the header's own arithmetic runs here; the expectations are the big-int model's, in the Python test.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../phase2-bn254_amd/csrc/curveu.hpp"

static bool word(uint32_t& w) { return std::scanf("%" SCNx32, &w) == 1; }

int main() {
  using namespace zk;
  static_assert(sizeof(XYZZU<FqParams>) == 36 * 4 && sizeof(XYZZ<Fq>) == 32 * 4 && sizeof(Fq) == 32, "word layouts");
  size_t n_cases = 0;
  uint32_t op;
  while (word(op)) {
    uint32_t n = 0, w[36];
    if (op == 0 && !word(n)) return 2;
    for (int i = 0; i < 36; ++i)
      if (!word(w[i])) return 2;
    XYZZU<FqParams> acc;
    std::memcpy(&acc, w, sizeof acc);
    XYZZ<Fq> rec;
    if (op == 0) {
      for (uint32_t k = 0; k < n; ++k) {
        uint32_t c[17];
        for (int i = 0; i < 17; ++i)
          if (!word(c[i])) return 2;
        Fq xy[2];
        std::memcpy(xy, c, sizeof xy);
        xyzzu_add_mixed(acc, xy[0], xy[1], c[16] != 0);
      }
      rec = xyzzu_to_r(acc);
    } else if (op == 1) {
      for (int i = 0; i < 36; ++i)
        if (!word(w[i])) return 2;
      XYZZU<FqParams> o;
      std::memcpy(&o, w, sizeof o);
      xyzzr_add(acc, o);
      rec = xyzzr_store(acc);
    } else {
      std::fprintf(stderr, "case %zu: unknown op %u\n", n_cases, op);
      return 2;
    }
    uint32_t out[68];
    std::memcpy(out, &acc, 36 * 4);
    std::memcpy(out + 36, &rec, 32 * 4);
    for (int i = 0; i < 68; ++i) std::printf(i ? " %08" PRIx32 : "%08" PRIx32, out[i]);
    std::printf("\n");
    ++n_cases;
  }
  return n_cases ? 0 : 2;
}
