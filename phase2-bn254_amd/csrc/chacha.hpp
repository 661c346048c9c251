// The ChaCha20 block function and the Fr scalar stream cut from its keystream, stated once for host and device (as pairing.hpp is): the
// random exponents rho of merge_pairs / power_pairs (powersoftau/src/utils.rs:112-135, phase2/src/utils.rs:59-105), which the reference
// draws from thread_rng and this library generates where they are used.  Plain C++: no inline assembly, no LDS, no lane communication.
//
// State (16 u32 words): 0..3 the constants "expand 32-byte k", 4..11 the key, 12 | 13 << 32 a 64-bit block counter, 14 | 15 << 32 a 64-bit
// stream id.  20 rounds (10 column + diagonal double rounds), then the input state is added word by word.
//
// THE SCALAR STREAM of (key, stream_id).  Scalar number g (a global 64-bit index) is taken from block g >> 1, words 8 (g & 1) ..
// 8 (g & 1) + 7: limb j = word[2 j] | word[2 j + 1] << 32, and the top limb is masked to 61 bits.  The value is uniform in [0, 2^253) and,
// because 2^253 < r (r >> 253 == 1), a canonical FrRepr without rejection.  Nothing else enters: not the launch geometry, not how a range
// is cut into calls.  The price of the mask is that the scalars cover 2^253 of the r residues; a random linear combination over them
// accepts a false statement with probability 2^-253 per check (the reference on its own generator, utils.rs:116: "we do not need to be
// overly cautious of the RNG used for this check").
#pragma once
#include <cstdint>

#if defined(__HIPCC__)
#define ZK_CHACHA_HD __host__ __device__ __forceinline__
#else
#define ZK_CHACHA_HD inline
#endif

namespace zk {

constexpr uint32_t CHACHA_C0 = 0x61707865u, CHACHA_C1 = 0x3320646eu, CHACHA_C2 = 0x79622d32u, CHACHA_C3 = 0x6b206574u;   // "expa" "nd 3" "2-by" "te k"
constexpr uint64_t FR_RANDOM_TOP_MASK = (1ull << 61) - 1;   // top limb: bits 192..252

ZK_CHACHA_HD uint32_t chacha_rotl(uint32_t v, int c) { return (v << c) | (v >> (32 - c)); }

#define ZK_CHACHA_QR(a, b, c, d)   \
  a += b; d ^= a; d = chacha_rotl(d, 16); \
  c += d; b ^= c; b = chacha_rotl(b, 12); \
  a += b; d ^= a; d = chacha_rotl(d, 8);  \
  c += d; b ^= c; b = chacha_rotl(b, 7);

// out[0..15] = the keystream words of block `counter` of (key, stream_id)
ZK_CHACHA_HD void chacha20_block(uint32_t out[16], const uint32_t key[8], uint64_t counter, uint64_t stream_id) {
  const uint32_t i12 = (uint32_t)counter, i13 = (uint32_t)(counter >> 32), i14 = (uint32_t)stream_id, i15 = (uint32_t)(stream_id >> 32);
  uint32_t x0 = CHACHA_C0, x1 = CHACHA_C1, x2 = CHACHA_C2, x3 = CHACHA_C3;
  uint32_t x4 = key[0], x5 = key[1], x6 = key[2], x7 = key[3], x8 = key[4], x9 = key[5], x10 = key[6], x11 = key[7];
  uint32_t x12 = i12, x13 = i13, x14 = i14, x15 = i15;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    ZK_CHACHA_QR(x0, x4, x8, x12)
    ZK_CHACHA_QR(x1, x5, x9, x13)
    ZK_CHACHA_QR(x2, x6, x10, x14)
    ZK_CHACHA_QR(x3, x7, x11, x15)
    ZK_CHACHA_QR(x0, x5, x10, x15)
    ZK_CHACHA_QR(x1, x6, x11, x12)
    ZK_CHACHA_QR(x2, x7, x8, x13)
    ZK_CHACHA_QR(x3, x4, x9, x14)
  }
  out[0] = x0 + CHACHA_C0;  out[1] = x1 + CHACHA_C1;  out[2] = x2 + CHACHA_C2;   out[3] = x3 + CHACHA_C3;
  out[4] = x4 + key[0];     out[5] = x5 + key[1];     out[6] = x6 + key[2];      out[7] = x7 + key[3];
  out[8] = x8 + key[4];     out[9] = x9 + key[5];     out[10] = x10 + key[6];    out[11] = x11 + key[7];
  out[12] = x12 + i12;      out[13] = x13 + i13;      out[14] = x14 + i14;       out[15] = x15 + i15;
}
#undef ZK_CHACHA_QR

// the two scalars of one block: lo[0..3] = scalar 2 * block, hi[0..3] = scalar 2 * block + 1 (canonical FrRepr limbs)
ZK_CHACHA_HD void fr_random_block(uint64_t lo[4], uint64_t hi[4], const uint32_t key[8], uint64_t stream_id, uint64_t block) {
  uint32_t w[16];
  chacha20_block(w, key, block, stream_id);
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lo[j] = (uint64_t)w[2 * j] | ((uint64_t)w[2 * j + 1] << 32);
    hi[j] = (uint64_t)w[8 + 2 * j] | ((uint64_t)w[8 + 2 * j + 1] << 32);
  }
  lo[3] &= FR_RANDOM_TOP_MASK;
  hi[3] &= FR_RANDOM_TOP_MASK;
}

}  // namespace zk
