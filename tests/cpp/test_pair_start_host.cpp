// xyzzu_from_affine_pair (csrc/curveu.hpp) compiled for the HOST, as a stand-alone program: tests/test_pair_start_host.py builds it with
// -fsanitize=undefined,address and feeds it the cases of tests/pair_start_vectors.py.
//   stdin : one case per line, 34 hexadecimal words: x1, y1, x2, y2 (canonical memory-format coordinates, 8 x 32 bits each), negate1, negate2
//   stdout: one line per case, 68 hexadecimal words: the accumulator (X, Y, ZZ, ZZZ, nine limbs each), then xyzzu_to_r of it (4 x 8 words)
// Nothing but the header's own arithmetic runs here; the expectations are the big-int model's, in the Python test.
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../phase2-bn254_amd/csrc/curveu.hpp"

int main() {
  using namespace zk;
  static_assert(sizeof(XYZZU<FqParams>) == 36 * 4 && sizeof(XYZZ<Fq>) == 32 * 4 && sizeof(Fq) == 32, "word layouts");
  uint32_t in[34];
  size_t n = 0;
  for (;;) {
    int got = 0;
    for (; got < 34; ++got)
      if (std::scanf("%" SCNx32, &in[got]) != 1) break;
    if (got == 0) break;
    if (got != 34) {
      std::fprintf(stderr, "case %zu: %d words, want 34\n", n, got);
      return 2;
    }
    Fq c[4];
    std::memcpy(c, in, sizeof(c));
    const XYZZU<FqParams> acc = xyzzu_from_affine_pair(c[0], c[1], in[32] != 0, c[2], c[3], in[33] != 0);
    const XYZZ<Fq> rec = xyzzu_to_r(acc);
    uint32_t out[68];
    std::memcpy(out, &acc, 36 * 4);
    std::memcpy(out + 36, &rec, 32 * 4);
    for (int i = 0; i < 68; ++i) std::printf(i ? " %08" PRIx32 : "%08" PRIx32, out[i]);
    std::printf("\n");
    ++n;
  }
  return n ? 0 : 2;
}
