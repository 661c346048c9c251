"""Key pairs, proofs of knowledge and the hash into G2 of both ceremonies: the once-per-contribution work the reference does on single
points, done here on the host as generator.py and pairing.py do theirs -- Python integers for the field work of hash_to_g2 and the
record codecs, the library's host helpers (mi355zk_bn254_g{1,2}_mul / _to_affine) for the scalar multiplications.

Mirrored interfaces (same names, argument meaning and order):
  powersoftau/src/utils.rs:31-45      hash_to_g2(digest)                                      (phase2/src/utils.rs:111-122 is the same function)
  powersoftau/src/utils.rs:172-185    compute_g2_s(digest, g1_s, g1_s_x, personalization)
  powersoftau/src/keypair.rs:54-103   keypair(rng, digest)            -> keypair(digest, tau, alpha, beta)
  powersoftau/src/keypair.rs:105-163  PublicKey::{serialize, deserialize}  -> write_public_key / read_public_key
  phase2/src/parameters.rs:860-908    keypair(rng, current)           -> mpc_keypair(mpc, delta)
  phase2/src/keypair.rs               PublicKey::write and its hash   -> mpc_public_key_bytes / mpc_public_key_hash

hash_to_g2 AND THE REFERENCE'S BYTES.  hash_to_g2 is `ChaChaRng::from_seed(first eight big-endian u32 of the digest).gen::<G2>()`.  What this
module pins, and the tests hold it to:
  - the ChaCha keystream: rand 0.4's ChaChaRng is ChaCha20 with the seed as key and a zero counter and nonce, read word by word
    (the same block function as csrc/chacha.hpp, held against the published keystream);
  - the structure of G2::rand (pairing/src/bn256/ec.rs:1091-1106): x: Fq2 = rng.gen() (c0 then c1, fq2.rs:103), greatest: bool = rng.gen(),
    get_point_from_x (:110-131: y chosen by (y < -y) ^ greatest, whichever root the square root returns; Fq2 ordered by c1 then c0,
    fq2.rs:21-30), the non-zero and on-curve tests, scale_by_cofactor with the literal of :1350-1355;
  - the draws as the project restates rand 0.4 / ff_derive for its seeded vectors (tests/bn254_model.py): next_u64 = high word first, an Fq
    = four next_u64 limbs, lowest first, top two bits cleared, redrawn until below q, the accepted value being the element's Montgomery
    representation; bool = the low bit of one next_u32;
  - membership: the result is a non-zero point of the twist in the order-r subgroup.
Byte compatibility with the Rust binaries is NOT tested: there is no Rust toolchain and no `rand` / `ff_derive` source to run against.  A
contribution made and verified with this library is self-consistent; whether the Rust verifier derives the same G2 point from the same
digest is unverified.

Points are raw affine records (numpy u64: 8 limbs for G1, 16 for G2, Montgomery form, all-zero = infinity), scalars Python ints mod r.
"""
from __future__ import annotations

import hashlib
import secrets

import numpy as np

from . import prover as _prover
from .ceremony import _R_ORDER, G1_ONE_RAW, DeserializationError, GroupDecodingError

_Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583   # fq.rs:5
_MONT_R = 1 << 256
_MONT_R_INV = pow(_MONT_R, -1, _Q)
_G2_COFACTOR = 0x30644E72E131A029B85045B68181585E06CEECDA572A2489345F2299C0F9FA8D   # ec.rs:1350-1355: 2 q - r
_B_G2 = None   # 3 / (9 + u), set below (fq.rs:18-31)
_M32 = 0xFFFFFFFF


# ---- ChaCha20 (the block function of csrc/chacha.hpp, on Python ints) and rand 0.4's ChaChaRng over it
def chacha20_block(key, counter: int, stream_id: int = 0):
    """The 16 keystream words of block `counter`: constants "expand 32-byte k", key in words 4..11, counter in 12, 13, stream_id in 14, 15."""
    init = [0x61707865, 0x3320646E, 0x79622D32, 0x6B206574, *[int(k) & _M32 for k in key],
            counter & _M32, (counter >> 32) & _M32, stream_id & _M32, (stream_id >> 32) & _M32]
    x = list(init)

    def qr(a, b, c, d):
        x[a] = (x[a] + x[b]) & _M32
        x[d] ^= x[a]
        x[d] = ((x[d] << 16) | (x[d] >> 16)) & _M32
        x[c] = (x[c] + x[d]) & _M32
        x[b] ^= x[c]
        x[b] = ((x[b] << 12) | (x[b] >> 20)) & _M32
        x[a] = (x[a] + x[b]) & _M32
        x[d] ^= x[a]
        x[d] = ((x[d] << 8) | (x[d] >> 24)) & _M32
        x[c] = (x[c] + x[d]) & _M32
        x[b] ^= x[c]
        x[b] = ((x[b] << 7) | (x[b] >> 25)) & _M32

    for _ in range(10):
        qr(0, 4, 8, 12), qr(1, 5, 9, 13), qr(2, 6, 10, 14), qr(3, 7, 11, 15)
        qr(0, 5, 10, 15), qr(1, 6, 11, 12), qr(2, 7, 8, 13), qr(3, 4, 9, 14)
    return [(a + b) & _M32 for a, b in zip(x, init)]


class ChaChaRng:
    """rand 0.4 ChaChaRng::from_seed(&[u32]) as a stream of words"""

    def __init__(self, seed):
        self._key = (list(seed) + [0] * 8)[:8]
        self._block, self._words = 0, iter(())

    def next_u32(self) -> int:
        for w in self._words:
            return w
        self._words = iter(chacha20_block(self._key, self._block))
        self._block += 1
        return next(self._words)

    def next_u64(self) -> int:
        hi = self.next_u32()
        return (hi << 32) | self.next_u32()

    def gen_fq(self) -> int:
        """the VALUE of a random Fq: the accepted 254-bit draw is the element's Montgomery representation"""
        while True:
            v = sum(self.next_u64() << (64 * i) for i in range(4)) & ((1 << 254) - 1)
            if v < _Q:
                return v * _MONT_R_INV % _Q

    def gen_bool(self) -> bool:
        return bool(self.next_u32() & 1)


# ---- Fq2 = Fq[u] / (u^2 + 1) on pairs of ints, and the twist in Jacobian coordinates
def _f2_mul(a, b):
    return ((a[0] * b[0] - a[1] * b[1]) % _Q, (a[0] * b[1] + a[1] * b[0]) % _Q)


def _f2_sqr(a):
    return ((a[0] + a[1]) * (a[0] - a[1]) % _Q, 2 * a[0] * a[1] % _Q)


def _f2_add(a, b):
    return ((a[0] + b[0]) % _Q, (a[1] + b[1]) % _Q)


def _f2_sub(a, b):
    return ((a[0] - b[0]) % _Q, (a[1] - b[1]) % _Q)


def _f2_neg(a):
    return (-a[0] % _Q, -a[1] % _Q)


def _f2_inv(a):
    n = pow(a[0] * a[0] + a[1] * a[1], -1, _Q)
    return (a[0] * n % _Q, -a[1] * n % _Q)


def _f2_pow(a, e: int):
    out = (1, 0)
    for bit in bin(e)[2:]:
        out = _f2_sqr(out)
        if bit == "1":
            out = _f2_mul(out, a)
    return out


_B_G2 = _f2_mul((3, 0), _f2_inv((9, 1)))


def _f2_sqrt(a):
    """fq2.rs:211-260 (Algorithm 9 of eprint 2012/685, q = 3 mod 4): a square root of a, or None"""
    if a == (0, 0):
        return (0, 0)
    a1 = _f2_pow(a, (_Q - 3) // 4)
    alpha = _f2_mul(_f2_sqr(a1), a)
    a0 = _f2_mul((alpha[0], -alpha[1] % _Q), alpha)      # alpha^q * alpha: the norm-one test
    if a0 == (_Q - 1, 0):
        return None
    x0 = _f2_mul(a1, a)
    if alpha == (_Q - 1, 0):
        return (-x0[1] % _Q, x0[0])                     # u * x0
    return _f2_mul(_f2_pow(_f2_add(alpha, (1, 0)), (_Q - 1) // 2), x0)


def _f2_less(a, b) -> bool:
    return (a[1], a[0]) < (b[1], b[0])   # fq2.rs:21-30: c1, then c0


def _jac_double(p):
    x, y, z = p
    if z == (0, 0):
        return p
    a, b = _f2_sqr(x), _f2_sqr(y)
    c = _f2_sqr(b)
    d = _f2_sub(_f2_sub(_f2_sqr(_f2_add(x, b)), a), c)
    d = _f2_add(d, d)
    e = _f2_add(_f2_add(a, a), a)
    x3 = _f2_sub(_f2_sqr(e), _f2_add(d, d))
    c8 = _f2_add(c, c)
    c8 = _f2_add(c8, c8)
    c8 = _f2_add(c8, c8)
    yz = _f2_mul(y, z)
    return (x3, _f2_sub(_f2_mul(e, _f2_sub(d, x3)), c8), _f2_add(yz, yz))


def _jac_add_affine(p, q):
    """p + q for an affine q that is not infinity"""
    x1, y1, z1 = p
    if z1 == (0, 0):
        return (q[0], q[1], (1, 0))
    z1z1 = _f2_sqr(z1)
    u2, s2 = _f2_mul(q[0], z1z1), _f2_mul(q[1], _f2_mul(z1, z1z1))
    if u2 == x1:
        return _jac_double(p) if s2 == y1 else ((0, 0), (1, 0), (0, 0))
    h, r = _f2_sub(u2, x1), _f2_sub(s2, y1)
    hh = _f2_sqr(h)
    hhh, v = _f2_mul(h, hh), _f2_mul(x1, hh)
    x3 = _f2_sub(_f2_sub(_f2_sqr(r), hhh), _f2_add(v, v))
    return (x3, _f2_sub(_f2_mul(r, _f2_sub(v, x3)), _f2_mul(y1, hhh)), _f2_mul(z1, h))


def _g2_mul_affine(p, k: int):
    """k * p on the twist by plain double-and-add from the top bit (mul_bits, ec.rs:88-103): valid for points OUTSIDE the subgroup too"""
    acc = ((0, 0), (1, 0), (0, 0))
    for bit in bin(k)[2:]:
        acc = _jac_double(acc)
        if bit == "1":
            acc = _jac_add_affine(acc, p)
    if acc[2] == (0, 0):
        return None
    zi = _f2_inv(acc[2])
    zi2 = _f2_sqr(zi)
    return (_f2_mul(acc[0], zi2), _f2_mul(acc[1], _f2_mul(zi2, zi)))


# ---- raw records <-> ints <-> the reference's uncompressed encoding
def _limbs(v: int):
    return [(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]


def _coords(rec) -> list:
    """the canonical coordinates of a raw affine record, in record order (x, y / x.c0, x.c1, y.c0, y.c1)"""
    rec = np.asarray(rec, dtype=np.uint64).reshape(-1)
    return [sum(int(v) << (64 * i) for i, v in enumerate(rec[4 * k:4 * k + 4])) * _MONT_R_INV % _Q for k in range(rec.size // 4)]


def _record(coords) -> np.ndarray:
    return np.array([w for c in coords for w in _limbs(c * _MONT_R % _Q)], dtype=np.uint64)


def _host(rec, width: int) -> np.ndarray:
    """one point as a (width,) u64 host record, from numpy or a (1, width) / (width,) int64 tensor"""
    if hasattr(rec, "cpu"):
        rec = rec.cpu().numpy()
    a = np.ascontiguousarray(rec)
    a = a.view(np.uint64) if a.dtype == np.int64 else a.astype(np.uint64)
    a = a.reshape(-1)
    if a.size != width:
        raise ValueError(f"expected one point of {width} limbs")
    return a


def point_to_uncompressed(rec) -> bytes:
    """EncodedPoint::from_affine of the uncompressed forms (ec.rs:827-840, 1214-1228): big-endian canonical coordinates, G2 as x.c1, x.c0,
    y.c1, y.c0; infinity = bit 6 of the first byte, all else zero"""
    rec = np.asarray(rec, dtype=np.uint64).reshape(-1)
    size = 8 * rec.size
    if not rec.any():
        return bytes([0x40]) + bytes(size - 1)
    c = _coords(rec)
    order = c if rec.size == 8 else [c[1], c[0], c[3], c[2]]
    return b"".join(v.to_bytes(32, "big") for v in order)


def point_from_uncompressed(data: bytes, group: int, index: int = 0) -> np.ndarray:
    """into_affine (checked) of one uncompressed record + the never-infinity rule of the public-key readers (keypair.rs:127-140)"""
    if len(data) != 64 * group:
        raise ValueError(f"an uncompressed G{group} point has {64 * group} bytes")
    if data[0] & 0x80:
        raise GroupDecodingError(7, index)              # UnexpectedCompressionMode
    if data[0] & 0x40:
        if data[0] & 0x3F or any(data[1:]):
            raise GroupDecodingError(8, index)          # UnexpectedInformation
        raise DeserializationError("PointAtInfinity in a public key")
    vals = [int.from_bytes(data[32 * k:32 * k + 32], "big") for k in range(2 * group)]
    if any(v >= _Q for v in vals):
        raise GroupDecodingError(6, index)              # CoordinateDecodingError
    if group == 1:
        x, y = vals
        if (y * y - x * x * x - 3) % _Q:
            raise GroupDecodingError(4, index)          # NotOnCurve
        return _record(vals)
    x, y = (vals[1], vals[0]), (vals[3], vals[2])
    if _f2_sub(_f2_sqr(y), _f2_add(_f2_mul(_f2_sqr(x), x), _B_G2)) != (0, 0):
        raise GroupDecodingError(4, index)
    return _record([x[0], x[1], y[0], y[1]])


# ---- the hash into G2
def hash_to_g2(digest: bytes) -> np.ndarray:
    """powersoftau/src/utils.rs:31-45: G2::rand over ChaChaRng seeded with the first eight big-endian u32 of `digest` (>= 32 bytes; the
    rest is ignored), as a raw affine G2 record.  See the module docstring for what is and is not pinned against the reference."""
    digest = bytes(digest)
    if len(digest) < 32:
        raise ValueError("hash_to_g2 needs at least 32 bytes")
    rng = ChaChaRng([int.from_bytes(digest[4 * i:4 * i + 4], "big") for i in range(8)])
    while True:
        x = (rng.gen_fq(), rng.gen_fq())
        greatest = rng.gen_bool()
        y = _f2_sqrt(_f2_add(_f2_mul(_f2_sqr(x), x), _B_G2))
        if y is None:
            continue
        neg = _f2_neg(y)
        y = y if _f2_less(y, neg) ^ greatest else neg
        # (non-zero: an affine point built from coordinates never is; on the curve: by construction -- ec.rs:1098-1099 cannot fail)
        p = _g2_mul_affine((x, y), _G2_COFACTOR)
        if p is None:
            continue
        return _record([p[0][0], p[0][1], p[1][0], p[1][1]])


def compute_g2_s(digest: bytes, g1_s, g1_s_x, personalization: int) -> np.ndarray:
    """utils.rs:172-185: hash_to_g2(BLAKE2b(personalization | digest | g1_s | g1_s_x)), the points uncompressed"""
    h = hashlib.blake2b(digest_size=64)
    h.update(bytes([personalization]))
    h.update(bytes(digest))
    h.update(point_to_uncompressed(_host(g1_s, 8)))
    h.update(point_to_uncompressed(_host(g1_s_x, 8)))
    return hash_to_g2(h.digest())


# ---- key pairs
def _random_scalar() -> int:
    return 1 + secrets.randbelow(_R_ORDER - 1)


def _mul_affine(rec: np.ndarray, k: int) -> np.ndarray:
    return _prover._to_affine(_prover._mul(rec, k))


PK_G1 = ("tau_g1_s", "tau_g1_s_tau", "alpha_g1_s", "alpha_g1_s_alpha", "beta_g1_s", "beta_g1_s_beta")
PK_G2 = ("tau_g2", "alpha_g2", "beta_g2")
PUBLIC_KEY_SIZE = 6 * 64 + 3 * 128


def keypair(digest: bytes, tau: int = None, alpha: int = None, beta: int = None):
    """keypair.rs:54-103 for a 64-byte transcript digest -> (public key, private key).  The public key is a dict of host records named as
    the deserialiser names them (tau_g1_s, tau_g1_s_tau, ..., tau_g2, alpha_g2, beta_g2); the private key {"tau", "alpha", "beta"} of ints,
    drawn from the `secrets` module when not given.  g1_s is a random multiple of the generator (G1::rand in the reference: not its
    byte stream, any non-zero point serves)."""
    digest = bytes(digest)
    if len(digest) != 64:
        raise ValueError("the transcript digest has 64 bytes")
    priv = {"tau": tau if tau is not None else _random_scalar(), "alpha": alpha if alpha is not None else _random_scalar(),
            "beta": beta if beta is not None else _random_scalar()}
    pub = {}
    for name, personalization in (("tau", 0), ("alpha", 1), ("beta", 2)):
        x = priv[name] % _R_ORDER
        g1_s = _mul_affine(G1_ONE_RAW, _random_scalar())
        g1_s_x = _mul_affine(g1_s, x)
        g2_s = compute_g2_s(digest, g1_s, g1_s_x, personalization)
        pub[f"{name}_g1_s"], pub[f"{name}_g1_s_{name}"], pub[f"{name}_g2"] = g1_s, g1_s_x, _mul_affine(g2_s, x)
    return pub, priv


def write_public_key(pub) -> bytes:
    """PublicKey::serialize (keypair.rs:107-122): six G1 and three G2 points, uncompressed"""
    return b"".join(point_to_uncompressed(_host(pub[k], 8)) for k in PK_G1) + b"".join(point_to_uncompressed(_host(pub[k], 16)) for k in PK_G2)


def read_public_key(data: bytes):
    """PublicKey::deserialize (keypair.rs:127-163): every point checked, none the point at infinity"""
    data = bytes(data)
    if len(data) != PUBLIC_KEY_SIZE:
        raise ValueError(f"a public key has {PUBLIC_KEY_SIZE} bytes")
    pub = {k: point_from_uncompressed(data[64 * i:64 * i + 64], 1, i) for i, k in enumerate(PK_G1)}
    for i, k in enumerate(PK_G2):
        pub[k] = point_from_uncompressed(data[384 + 128 * i:384 + 128 * i + 128], 2, 6 + i)
    return pub


# ---- phase 2
def mpc_public_key_bytes(pk) -> bytes:
    """PublicKey::write (phase2): delta_after, s, s_delta (G1), r_delta (G2), uncompressed, then the 64-byte transcript"""
    t = pk["transcript"]
    t = bytes(t.cpu().numpy()) if hasattr(t, "cpu") else bytes(t)
    return (point_to_uncompressed(_host(pk["delta_after"], 8)) + point_to_uncompressed(_host(pk["s"], 8)) + point_to_uncompressed(_host(pk["s_delta"], 8))
            + point_to_uncompressed(_host(pk["r_delta"], 16)) + t)


def mpc_public_key_hash(pk) -> bytes:
    """what MPCParameters::contribute returns and verify / verify_contribution report (parameters.rs:512-521): BLAKE2b of the public key"""
    return hashlib.blake2b(mpc_public_key_bytes(pk), digest_size=64).digest()


def mpc_transcript(cs_hash: bytes, contributions, s, s_delta) -> bytes:
    """H(cs_hash | <previous pubkeys> | s | s_delta) (parameters.rs:872-885)"""
    h = hashlib.blake2b(digest_size=64)
    h.update(bytes(cs_hash))
    for pk in contributions:
        h.update(mpc_public_key_bytes(pk))
    h.update(point_to_uncompressed(_host(s, 8)))
    h.update(point_to_uncompressed(_host(s_delta, 8)))
    return h.digest()


def mpc_keypair(mpc, delta: int = None):
    """phase2 keypair (parameters.rs:860-908) over the dict ceremony.read_mpc_parameters / circom.mpc_parameters_new return -> (public key,
    delta).  The public key holds host records (delta_after, s, s_delta: 8 limbs; r_delta: 16) and the 64-byte transcript."""
    delta = (delta if delta is not None else _random_scalar()) % _R_ORDER
    if delta == 0:
        raise ValueError("delta must be non-zero")
    cs_hash = mpc["cs_hash"]
    cs_hash = bytes(cs_hash.cpu().numpy()) if hasattr(cs_hash, "cpu") else bytes(cs_hash)
    s = _mul_affine(G1_ONE_RAW, _random_scalar())
    s_delta = _mul_affine(s, delta)
    transcript = mpc_transcript(cs_hash, mpc["contributions"], s, s_delta)
    r = hash_to_g2(transcript)
    pub = {"delta_after": _mul_affine(_host(mpc["params"]["vk"]["delta_g1"], 8), delta), "s": s, "s_delta": s_delta, "r_delta": _mul_affine(r, delta),
           "transcript": transcript}
    return pub, delta
