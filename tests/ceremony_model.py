"""Independent Python model of the ceremony-side additions (TEST INFRASTRUCTURE ONLY; shares no code with the library or with
phase2-bn254_amd/keys.py):

  - ChaCha20 as RFC 7539 section 2.3 states the block function, over a list of 16 ints, with the library's state layout: the constants
    "expand 32-byte k", the key in words 4..11, a 64-bit block counter in words 12, 13 and a 64-bit stream id in words 14, 15;
  - the Fr scalar stream cut from it (include/mi355zk.h: scalar g = words 8 (g & 1) .. 8 (g & 1) + 7 of block g >> 1, top limb 61 bits);
  - rand 0.4's ChaChaRng as a word stream (from_seed: the seed is the key, counter and stream id zero), next_u64 = high word first, the
    field and bool draws as tests/bn254_model.py restates them for XorShiftRng;
  - hash_to_g2 (powersoftau/src/utils.rs:31-45) = G2::rand (pairing/src/bn256/ec.rs:1091-1106) over that generator, on bn254_model's
    affine big-int curve code, with a square root in Fq2 by the norm method (the library side uses the exponentiation of fq2.rs:211).
"""
from __future__ import annotations

import bn254_model as M

MASK32 = 0xFFFFFFFF
SIGMA = (0x61707865, 0x3320646E, 0x79622D32, 0x6B206574)
G2_COFACTOR = 0x30644E72E131A029B85045B68181585E06CEECDA572A2489345F2299C0F9FA8D   # ec.rs:1350-1355 (= 2 q - r)


def _rotl(v, c):
    return ((v << c) & MASK32) | (v >> (32 - c))


def _quarter(s, a, b, c, d):
    s[a] = (s[a] + s[b]) & MASK32; s[d] = _rotl(s[d] ^ s[a], 16)   # noqa: E702
    s[c] = (s[c] + s[d]) & MASK32; s[b] = _rotl(s[b] ^ s[c], 12)   # noqa: E702
    s[a] = (s[a] + s[b]) & MASK32; s[d] = _rotl(s[d] ^ s[a], 8)    # noqa: E702
    s[c] = (s[c] + s[d]) & MASK32; s[b] = _rotl(s[b] ^ s[c], 7)    # noqa: E702


def chacha20_block(key, counter: int, stream_id: int = 0):
    """the 16 keystream words of one block"""
    init = list(SIGMA) + [int(k) & MASK32 for k in key] + [counter & MASK32, (counter >> 32) & MASK32, stream_id & MASK32, (stream_id >> 32) & MASK32]
    assert len(init) == 16
    s = list(init)
    for _ in range(10):
        for idx in ((0, 4, 8, 12), (1, 5, 9, 13), (2, 6, 10, 14), (3, 7, 11, 15), (0, 5, 10, 15), (1, 6, 11, 12), (2, 7, 8, 13), (3, 4, 9, 14)):
            _quarter(s, *idx)
    return [(a + b) & MASK32 for a, b in zip(s, init)]


def fr_random(key, stream_id: int, first: int, n: int):
    """scalars first .. first + n - 1 as lists of four u64 limbs"""
    out = []
    for g in range(first, first + n):
        w = chacha20_block(key, g >> 1, stream_id)[8 * (g & 1):8 * (g & 1) + 8]
        limbs = [w[2 * j] | (w[2 * j + 1] << 32) for j in range(4)]
        limbs[3] &= (1 << 61) - 1
        out.append(limbs)
    return out


class ChaChaRng:
    def __init__(self, seed):
        self.key = list(seed) + [0] * (8 - len(seed))
        self.block, self.buf = 0, []

    def next_u32(self) -> int:
        if not self.buf:
            self.buf = chacha20_block(self.key, self.block, 0)
            self.block += 1
        return self.buf.pop(0)

    def next_u64(self) -> int:
        hi = self.next_u32()
        return (hi << 32) | self.next_u32()

    def gen_fq(self) -> int:
        """the value of the field element whose Montgomery representation is the accepted 254-bit draw"""
        while True:
            v = 0
            for i in range(4):
                v |= self.next_u64() << (64 * i)
            v &= (1 << 254) - 1
            if v < M.Q:
                return M.from_mont(v, M.Q)

    def gen_bool(self) -> bool:
        return bool(self.next_u32() & 1)


def _fq_sqrt(a: int):
    r = pow(a, (M.Q + 1) // 4, M.Q)   # q = 3 mod 4
    return r if r * r % M.Q == a % M.Q else None


def f2_sqrt(a):
    """a square root of a = a0 + a1 u in Fq[u] / (u^2 + 1) through the norm, or None"""
    a0, a1 = a
    if a1 == 0:
        r = _fq_sqrt(a0)
        if r is not None:
            return (r, 0)
        r = _fq_sqrt(-a0 % M.Q)    # sqrt(-1) = u
        return (0, r)
    n = _fq_sqrt((a0 * a0 + a1 * a1) % M.Q)
    if n is None:
        return None
    inv2 = pow(2, -1, M.Q)
    for nn in (n, -n % M.Q):
        x0 = _fq_sqrt((a0 + nn) * inv2 % M.Q)
        if x0 is not None and x0 != 0:
            x1 = a1 * pow(2 * x0, -1, M.Q) % M.Q
            if M.f2_mul((x0, x1), (x0, x1)) == (a0 % M.Q, a1 % M.Q):
                return (x0, x1)
    return None


def _f2_less(a, b) -> bool:
    """fq2.rs:21-30: c1 decides, then c0"""
    return (a[1], a[0]) < (b[1], b[0])


def hash_to_g2(digest: bytes):
    """affine ((x0, x1), (y0, y1)) of canonical ints"""
    assert len(digest) >= 32
    rng = ChaChaRng([int.from_bytes(digest[4 * i:4 * i + 4], "big") for i in range(8)])
    while True:
        x = (rng.gen_fq(), rng.gen_fq())
        greatest = rng.gen_bool()
        y = f2_sqrt(M.f2_add(M.f2_mul(M.f2_mul(x, x), x), M.B_G2))
        if y is None:
            continue
        neg = M.f2_neg(y)
        p = (x, y if _f2_less(y, neg) ^ greatest else neg)
        assert M.on_curve_g2(p)
        return M.ec_mul(M.FQ2_OPS, p, G2_COFACTOR)
