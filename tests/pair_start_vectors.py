"""Operands and big-int expectations for xyzzu_from_affine_pair (csrc/curveu.hpp): how a G1 bucket opens.

TEST INFRASTRUCTURE, plain Python, no GPU.  Both legs import it: tests/test_pair_start_host.py (the host build of the header under
AddressSanitizer / UBSan, a stand-alone program) and tests/test_gpu_pair_start_op.py (MI355ZK_DEVOP_G1_ADD_AFFINE_PAIR on the device).

A case is 34 words: x1, y1, x2, y2 as canonical memory-format coordinates (value * 2^256 mod p, 8 x 32 bits) and the two sign words.
The result is 68 words: the accumulator (X, Y, ZZ, ZZZ on nine 29-bit limbs) and xyzzu_to_r of it (four canonical coordinates).
"""
from __future__ import annotations

import random

import bn254_model as M
import field_edge_vectors as V

IN_WORDS, OUT_WORDS = 34, 68
CODE = len(V.ALL_OPS)    # MI355ZK_DEVOP_G1_ADD_AFFINE_PAIR = MI355ZK_DEVOP_COUNT (include/mi355zk.h: the first code after the table's ops)
N_RANDOM = 64            # random pairs, each under all four sign combinations
G = V.G1
Q = M.Q


def _sqrt(a):
    r = pow(a, (Q + 1) // 4, Q)          # q = 3 mod 4
    return r if r * r % Q == a % Q else None


def _cbrt(a):
    """a cube root of a mod q, or None (q = 1 mod 3: one value in three has roots; found through a generator-free search of the cofactor power)"""
    if a % Q == 0:
        return 0
    if pow(a, (Q - 1) // 3, Q) != 1:
        return None
    # q - 1 = 3^s * t, t coprime to 3: a^(inverse of 3 mod t) is a root up to an element of the 3-Sylow group; search that group
    s, t = 0, Q - 1
    while t % 3 == 0:
        s, t = s + 1, t // 3
    r = pow(a, pow(3, -1, t), Q)
    g = next(pow(z, t, Q) for z in range(2, 100) if pow(z, (Q - 1) // 3, Q) != 1)   # generates the 3-Sylow group
    for k in range(3 ** s):
        if pow(r, 3, Q) == a % Q:
            return r
        r = r * g % Q
    return None


def point_with_x_near(x0, step):
    """the curve point (smaller y) whose x is x0, or the nearest x in direction `step` that has one"""
    x = x0 % Q
    while True:
        y = _sqrt((x * x * x + M.B_G1) % Q)
        if y:
            return (x, min(y, Q - y))
        x = (x + step) % Q


def point_with_y_near(y0, step):
    y = y0 % Q
    while True:
        x = _cbrt((y * y - M.B_G1) % Q)
        if x is not None and y != 0:
            return (x, y)
        y = (y + step) % Q


def edge_points():
    """x or y equal to 0, 1, p - 1 where the curve has such a point, else the nearest coordinate that has one (y = 0 never has)"""
    out = []
    for name, v, step in (("0", 0, 1), ("1", 1, 1), ("p-1", Q - 1, -1)):
        px = point_with_x_near(v, step)
        out.append(("x%s%s" % ("=" if px[0] == v else "~", name), px))
        py = point_with_y_near(v if v else 3, step)      # (y = 1 is a case of its own, y = 2 belongs to the point with x = 1)
        out.append(("y%s%s" % ("=" if py[1] == v else "~", name), py))
    for _, pt in out:
        assert M.on_curve_g1(pt)
    return out


def case_words(p1, n1, p2, n2):
    return G.coord_words(p1[0]) + G.coord_words(p1[1]) + G.coord_words(p2[0]) + G.coord_words(p2[1]) + [int(n1), int(n2)]


def cases():
    """[(name, 34 input words, expected affine point or None)]"""
    rnd = random.Random(0x9A1F_57A7)
    named, more = V.pool(G)
    edges = edge_points()
    rows = []

    def add(name, p1, n1, p2, n2):
        a = M.ec_neg(M.FQ_OPS, p1) if n1 else p1
        b = M.ec_neg(M.FQ_OPS, p2) if n2 else p2
        rows.append((name, case_words(p1, n1, p2, n2), M.ec_add(M.FQ_OPS, a, b)))

    signs = ((0, 0), (0, 1), (1, 0), (1, 1))
    for i in range(N_RANDOM):
        a, b = rnd.sample(more, 2)
        for n1, n2 in signs:
            add("random %d %s%s" % (i, "+-"[n1], "+-"[n2]), a, n1, b, n2)
    others = [pt for _, pt in named[:5]] + more[:3]
    for en, e in edges:
        for k, o in enumerate(others):
            for n1, n2 in signs:
                add("%s first, other %d %s%s" % (en, k, "+-"[n1], "+-"[n2]), e, n1, o, n2)
                add("%s second, other %d %s%s" % (en, k, "+-"[n1], "+-"[n2]), o, n1, e, n2)
    for (na, a), (nb, b) in ((x, y) for x in edges for y in edges if x[0] != y[0]):
        n1, n2 = rnd.choice(signs)
        add("%s with %s %s%s" % (na, nb, "+-"[n1], "+-"[n2]), a, n1, b, n2)
    for n, pt in named[:5] + edges + [("random", more[5]), ("random", more[6])]:
        add("P, P ++ (doubles) " + n, pt, 0, pt, 0)
        add("P, P -- (doubles) " + n, pt, 1, pt, 1)
        add("P, P +- (infinity) " + n, pt, 0, pt, 1)
        add("P, P -+ (infinity) " + n, pt, 1, pt, 0)
        add("P, -P ++ (infinity) " + n, pt, 0, M.ec_neg(M.FQ_OPS, pt), 0)
        add("P, -P -- (infinity) " + n, pt, 1, M.ec_neg(M.FQ_OPS, pt), 1)
        add("P, -P +- (doubles) " + n, pt, 0, M.ec_neg(M.FQ_OPS, pt), 1)
    return rows


def verify(name, outw, want):
    """the accumulator is the expected point under the invariants of curveu.hpp (N-form, X < 6p, Y, ZZ, ZZZ < 2p, ZZ^3 == ZZZ^2; infinity:
    literal-zero ZZ) and the record is xyzzu_to_r of exactly that accumulator -- V.dec_point asserts the invariants"""
    outw = [int(x) for x in outw]
    assert len(outw) == OUT_WORDS
    acc, rec = outw[:36], outw[36:]
    try:
        pt, vals = V.dec_point(G, acc, 266)
        assert pt == want, "got %s, want %s" % (pt, want)
        if want is None:
            assert not any(rec), "infinity must give the zero record"
        else:
            V.BY_NAME["G1_ADD_MIXED"]._rec_check(vals, rec, pow(32, -1, Q))
    except AssertionError as e:
        raise AssertionError("%s: %s\n  acc %s" % (name, e, V.hexw(acc))) from None
