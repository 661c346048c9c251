"""Operands and big-int expectations for xyzzu_add_mixed, xyzzr_add and xyzzu_to_r / xyzzr_store (csrc/curveu.hpp) on the HOST build.

TEST INFRASTRUCTURE, plain Python, no GPU (tests/test_mixed_add_trim_host.py feeds tests/cpp/test_mixed_add_trim_host.cpp with it).

The formulas are polynomial identities mod p, so an accumulator need not be a curve point: it is INJECTED at the edges of the stated
invariants (X just below 6p; Y, ZZ, ZZZ just below 2p; limbs 0..7 all ones or all zero with limb 8 at both ends) and the result is
compared coordinate by coordinate with the same formula on big integers, in the domains of curveu.hpp:
    loaded x2, y2: value * 2^256      X, Y: value * 2^261      ZZ, ZZZ: value * 2^266 (bucket accumulator) or 2^261 (register form of a record)
"""
from __future__ import annotations

import random

import bn254_model as M
import field_edge_vectors as V

Q = M.Q
MASK = (1 << 29) - 1
I256, I261, I266, I32 = (pow(pow(2, e, Q), -1, Q) for e in (256, 261, 266, 5))


def limbs(v):
    assert 0 <= v < 1 << 264
    return [(v >> (29 * i)) & MASK for i in range(8)] + [v >> 232]


def value(l):
    return sum(x << (29 * i) for i, x in enumerate(l))


def words(v):
    return [(v >> (32 * i)) & 0xFFFFFFFF for i in range(8)]


def acc_words(vals):
    return [w for v in vals for w in limbs(v)]


def edge_values(k):
    """raw integers below k p at the edges of N-form: just below k p; limbs 0..7 all ones / all zero with limb 8 at both ends"""
    top = (k * Q - 1) >> 232
    return [k * Q - 1, k * Q - 2, (1 << 232) - 1, (((top - 1) << 232) | ((1 << 232) - 1)), top << 232, 1 << 232, 1, Q, Q - 1, Q + 1]


# ---- the model: field values (x, y, zz, zzz) with the powers of two taken out, or None for infinity ----
def dbl_affine(x, y):
    u = 2 * y % Q
    v = u * u % Q
    w = u * v % Q
    s = x * v % Q
    m = 3 * x * x % Q
    x3 = (m * m - 2 * s) % Q
    return (x3, (m * (s - x3) - w * y) % Q, v, w)


def dbl(a):
    x, y, zz, zzz = a
    x3, y3, v, w = dbl_affine(x, y)
    return (x3, y3, v * zz % Q, w * zzz % Q)


def add_mixed(a, x2, y2):
    if a is None:
        return (x2, y2, 1, 1)
    x1, y1, zz, zzz = a
    p = (x2 * zz - x1) % Q
    r = (y2 * zzz - y1) % Q
    if p == 0:
        return dbl_affine(x2, y2) if r == 0 else None
    pp = p * p % Q
    ppp = p * pp % Q
    q = x1 * pp % Q
    x3 = (r * r - ppp - 2 * q) % Q
    return (x3, (r * (q - x3) - y1 * ppp) % Q, zz * pp % Q, zzz * ppp % Q)


def add_full(a, b):
    if b is None:
        return a
    if a is None:
        return b
    u1, u2 = a[0] * b[2] % Q, b[0] * a[2] % Q
    s1, s2 = a[1] * b[3] % Q, b[1] * a[3] % Q
    p, r = (u2 - u1) % Q, (s2 - s1) % Q
    if p == 0:
        return dbl(a) if r == 0 else None
    pp = p * p % Q
    ppp = p * pp % Q
    q = u1 * pp % Q
    x3 = (r * r - ppp - 2 * q) % Q
    return (x3, (r * (q - x3) - s1 * ppp) % Q, a[2] * b[2] * pp % Q, a[3] * b[3] * ppp % Q)


def pair_start(x1, y1, x2, y2):
    """xyzzu_from_affine_pair: the sum of two affine points taken with Z = (x2 - x1) * 2^-5 (curveu.hpp)"""
    p, r = (x2 - x1) % Q, (y2 - y1) % Q
    if p == 0:
        return dbl_affine(x2, y2) if r == 0 else None
    pp = p * p % Q
    ppp = p * pp % Q
    q = x1 * pp % Q
    x3 = (r * r - ppp - 2 * q) % Q
    i10, i15 = I32 * I32 % Q, I32 * I32 * I32 % Q
    return (x3 * i10 % Q, (r * (q - x3) - y1 * ppp) % Q * i15 % Q, pp * i10 % Q, ppp * i15 % Q)


R261 = pow(2, 261, Q)


def bucket_record(points):
    """the record (16 u64: X, Y, ZZ, ZZZ canonical in the 2^261 domain) of a bucket whose signed affine points (x, y field values, identities left
    out) are added in list order the way accumulate_run does for a fresh lane-per-bucket launch: the first two by the pair start, the rest mixed"""
    a, k = None, 0
    if len(points) >= 2:
        a, k = pair_start(*points[0], *points[1]), 2
    for x, y in points[k:]:
        a = add_mixed(a, x, y)
    if a is None:
        return [0] * 16
    out = []
    for v in a:
        v = v * R261 % Q
        out += [(v >> (64 * i)) & 0xFFFFFFFFFFFFFFFF for i in range(4)]
    return out


def decode(raw, zdom):
    """raw integers (X, Y, ZZ, ZZZ) -> field values, None for the literal-zero ZZ"""
    if raw[2] == 0:
        return None
    return (raw[0] * I261 % Q, raw[1] * I261 % Q, raw[2] * zdom % Q, raw[3] * zdom % Q)


def cases():
    """[(name, input words, op, expected field values or None)]"""
    rnd = random.Random(0x7A1D_0D15)
    named, more = V.pool(V.G1)
    pts = [pt for _, pt in named[:5]] + more
    rows = []

    def loaded(v):   # memory words of the raw integer v, and the field value they stand for
        return words(v), v * I256 % Q

    def mixed(name, raw, adds):
        inw = [0, len(adds)] + acc_words(raw)
        a = decode(raw, I266)
        for xr, yr, neg in adds:
            (xw, xv), (yw, yv) = loaded(xr), loaded(yr)
            inw += xw + yw + [int(neg)]
            a = add_mixed(a, xv, (-yv) % Q if neg else yv)
        rows.append((name, inw, 0, a))

    def mem(pt):     # raw integers of a curve point's memory words
        return (pt[0] << 256) % Q, (pt[1] << 256) % Q

    def acc_of(pt, z, zbits):   # the accumulator (or register form, zbits = 261) holding pt with Z = z
        zz, zzz = z * z % Q, z * z * z % Q
        return [(pt[0] * zz << 261) % Q, (pt[1] * zzz << 261) % Q, (zz << zbits) % Q, (zzz << zbits) % Q]

    # injected accumulators at the edges of the invariants x loaded operands 0, 1, p - 1 and random points, both signs
    ex, ey = edge_values(6), edge_values(2)
    ops = [0, 1, Q - 1]
    label = {0: "0", 1: "1", Q - 1: "p-1"}
    k = 0
    for X in ex:
        for Y in ey:
            zz, zzz = ey[k % len(ey)], ey[(k // 3 + 1) % len(ey)]
            if zz % Q == 0 or zzz % Q == 0:
                zz, zzz = ey[0], ey[1]
            xr, yr = (ops[k % 3], ops[(k // 3) % 3]) if k % 2 else mem(pts[k % len(pts)])
            for neg in (0, 1):
                mixed("edge accumulator %d %s" % (k, "+-"[neg]), [X, Y, zz, zzz], [(xr, yr, neg)])
            k += 1
    for xr in ops:
        for yr in ops:
            for neg in (0, 1):
                mixed("operand x=%s y=%s %s on a random accumulator" % (label[xr], label[yr], "+-"[neg]), [rnd.randrange(6 * Q), rnd.randrange(2 * Q), rnd.randrange(1, 2 * Q), rnd.randrange(2 * Q)], [(xr, yr, neg)])
                mixed("operand x=%s y=%s %s on the empty accumulator" % (label[xr], label[yr], "+-"[neg]), [0, 0, 0, 0], [(xr, yr, neg)])
    # equal x: the same point doubles, the opposite point gives infinity; whichever way the signs say it
    for i, pt in enumerate(pts[:8]):
        z = rnd.randrange(1, Q)
        neg_pt = (pt[0], Q - pt[1])
        for name, held, added, neg in (("P + P", pt, pt, 0), ("P - (-P)", pt, neg_pt, 1), ("P - P", pt, pt, 1), ("P + (-P)", pt, neg_pt, 0), ("-P - P", neg_pt, pt, 1)):
            mixed("equal x %d: %s" % (i, name), acc_of(held, z, 266), [mem(added) + (neg,)])
    # chains: the un-carried D and the signed R are consumed many times; repeats give P + P and P - P on the way
    for c in range(3):
        adds, prev = [], pts[c]
        for j in range(80):
            pt = pts[rnd.randrange(len(pts))] if j % 9 != 1 else prev      # entries 1, 10, 19, ... repeat their predecessor
            prev = pt
            adds.append(mem(pt) + (rnd.randrange(2),))
        start = [0, 0, 0, 0] if c < 2 else [ex[0], ey[0], ey[1], ey[0]]
        mixed("chain %d of %d" % (c, len(adds)), start, adds)
    # xyzzr_add: register forms at the edges, random, equal and opposite points
    def full(name, ra, rb):
        rows.append((name, [1] + acc_words(ra) + acc_words(rb), 1, add_full(decode(ra, I261), decode(rb, I261))))

    for i, X in enumerate(ex):
        for j, Y in enumerate(ey[:6]):
            full("records at the edges %d %d" % (i, j), [X, Y, ey[(i + j) % 6], ey[(i + 2 * j + 1) % 6]], [ex[(i + 3) % len(ex)], ey[(j + 2) % 6], ey[(i + 1) % 6], ey[j]])
    for i in range(24):
        full("random records %d" % i, [rnd.randrange(6 * Q), rnd.randrange(2 * Q), rnd.randrange(1, 2 * Q), rnd.randrange(2 * Q)],
             [rnd.randrange(6 * Q), rnd.randrange(2 * Q), rnd.randrange(1, 2 * Q), rnd.randrange(2 * Q)])
    for i, pt in enumerate(pts[:6]):
        z1, z2 = rnd.randrange(1, Q), rnd.randrange(1, Q)
        full("the same point %d" % i, acc_of(pt, z1, 261), acc_of(pt, z2, 261))
        full("opposite points %d" % i, acc_of(pt, z1, 261), acc_of((pt[0], Q - pt[1]), z2, 261))
        full("infinity second %d" % i, acc_of(pt, z1, 261), [0, 0, 0, 0])
        full("infinity first %d" % i, [0, 0, 0, 0], acc_of(pt, z2, 261))
    return rows


def verify(name, op, outw, want):
    outw = [int(x) for x in outw]
    assert len(outw) == 68, name
    acc, rec = outw[:36], outw[36:]
    raw = [value(acc[9 * i:9 * i + 9]) for i in range(4)]
    try:
        if want is None:
            assert raw[2] == 0 and not any(rec), "infinity: literal-zero ZZ and the zero record"
            return
        assert all(x <= MASK for i in range(4) for x in acc[9 * i:9 * i + 8]), "N-form"
        assert raw[0] < 6 * Q and all(v < 2 * Q for v in raw[1:]), "X < 6p; Y, ZZ, ZZZ < 2p"
        got = decode(raw, I266 if op == 0 else I261)
        assert got == want, "coordinates differ from the big-int formula"
        close = I32 if op == 0 else 1        # xyzzu_to_r takes ZZ, ZZZ from the 2^266 to the 2^261 domain
        exp = words(raw[0] % Q) + words(raw[1] % Q) + words(raw[2] * close % Q) + words(raw[3] * close % Q)
        assert rec == exp, "record"
    except AssertionError as e:
        raise AssertionError("%s: %s\n  acc %s" % (name, e, V.hexw(acc))) from None
