"""Independent Python big-int model of the BN254 optimal ate pairing and of the Fq12 tower behind it.

TEST INFRASTRUCTURE ONLY.  It shares the tower and the basis of phase2-bn254_amd/csrc/pairing.hpp (they fix the bytes of a GT value)
and none of its formulas:
  - an Fq12 element is the polynomial a_0 + a_1 w + ... + a_5 w^5 over Fq2 with w^6 = xi = 9 + u; the product is the schoolbook
    product of two such polynomials (36 Fq2 products), no Karatsuba, no sparse forms;
  - the tower of the library, Fq6 = Fq2[v]/(v^3 - xi) and Fq12 = Fq6[w]/(w^2 - v), is the same ring with v = w^2:
    c0 = (a_0, a_2, a_4), c1 = (a_1, a_3, a_5) -- `to_tower` / `from_tower` reorder, nothing else;
  - the Frobenius map comes from its definition on the basis, (a_i w^i)^(q^k) = conj^k(a_i) * xi^(i (q^k - 1) / 6) * w^i, the constants
    computed here by square-and-multiply in Fq2 (test_pairing_host.py compares them with plain powering);
  - inverses go through norms (a * a^(q^6) lies in Fq6, b * b^(q^2) * b^(q^4) in Fq2), not through the cofactor formulas of the library;
  - the Miller loop keeps T AFFINE on the twist, walks the plain binary expansion of 6u + 2 (no NAF: the Miller function of an integer
    does not depend on the addition chain, up to factors in proper subfields which the final exponentiation removes), evaluates each line
    as a full Fq12 element and multiplies it in with the dense product;
  - the final exponentiation is one square-and-multiply by (q^12 - 1) / r.
One pairing takes a fraction of a second, a thousand would not: the tests use it sparingly and keep its results in tests/golden/pairing_golden.json.
"""
from __future__ import annotations

import bn254_model as M

Q = M.Q
R_ORDER = M.R_ORDER
BN_U = 4965661367192848881
ATE_LOOP = 6 * BN_U + 2
XI = (9, 1)
FINAL_EXPONENT = (Q ** 12 - 1) // R_ORDER
assert (Q ** 12 - 1) % R_ORDER == 0
assert Q == 36 * BN_U ** 4 + 36 * BN_U ** 3 + 24 * BN_U ** 2 + 6 * BN_U + 1 and R_ORDER == 36 * BN_U ** 4 + 36 * BN_U ** 3 + 18 * BN_U ** 2 + 6 * BN_U + 1

f2_add, f2_sub, f2_neg, f2_mul, f2_inv = M.f2_add, M.f2_sub, M.f2_neg, M.f2_mul, M.f2_inv
F2_ZERO, F2_ONE = (0, 0), (1, 0)


def f2_conj(a):
    return (a[0], (-a[1]) % Q)


def f2_pow(a, e: int):
    r = F2_ONE
    while e:
        if e & 1:
            r = f2_mul(r, a)
        a = f2_mul(a, a)
        e >>= 1
    return r


# ---------------------------------------------------------------- Fq12 = Fq2[w] / (w^6 - xi): tuples of six Fq2
ZERO = (F2_ZERO,) * 6
ONE = (F2_ONE,) + (F2_ZERO,) * 5


def f12_add(a, b):
    return tuple(f2_add(x, y) for x, y in zip(a, b))


def f12_sub(a, b):
    return tuple(f2_sub(x, y) for x, y in zip(a, b))


def f12_neg(a):
    return tuple(f2_neg(x) for x in a)


def f12_mul(a, b):
    acc = [[0, 0] for _ in range(11)]
    for i, (x0, x1) in enumerate(a):
        if x0 == 0 and x1 == 0:
            continue
        for j, (y0, y1) in enumerate(b):
            t = acc[i + j]
            t[0] += x0 * y0 - x1 * y1
            t[1] += x0 * y1 + x1 * y0
    out = []
    for k in range(6):
        c0, c1 = acc[k]
        if k < 5:
            h0, h1 = acc[k + 6]                      # w^(k+6) = xi w^k, xi = 9 + u
            c0 += 9 * h0 - h1
            c1 += 9 * h1 + h0
        out.append((c0 % Q, c1 % Q))
    return tuple(out)


def f12_sqr(a):
    return f12_mul(a, a)


def f12_pow(a, e: int):
    r = ONE
    for bit in bin(e)[2:]:
        r = f12_mul(r, r)
        if bit == "1":
            r = f12_mul(r, a)
    return r


def frobenius_constant(i: int, k: int):
    """xi^(i (q^k - 1) / 6): what w^i picks up under x -> x^(q^k)"""
    assert (Q ** k - 1) % 6 == 0
    return f2_pow(XI, i * (Q ** k - 1) // 6)


_FROB = {}


def f12_frobenius(a, k: int):
    k %= 12
    if k not in _FROB:
        _FROB[k] = [frobenius_constant(i, k) for i in range(6)]
    cs = _FROB[k]
    return tuple(f2_mul(f2_conj(x) if k & 1 else x, cs[i]) for i, x in enumerate(a))


def f12_conjugate(a):
    """x -> x^(q^6): w -> -w"""
    return tuple(f2_neg(x) if i & 1 else x for i, x in enumerate(a))


def f12_inv(a):
    n6 = f12_mul(a, f12_conjugate(a))                # in Fq6: odd coefficients vanish
    assert all(n6[i] == F2_ZERO for i in (1, 3, 5))
    co = f12_mul(f12_frobenius(n6, 2), f12_frobenius(n6, 4))
    n2 = f12_mul(n6, co)                             # the norm of n6 over Fq2
    assert all(x == F2_ZERO for x in n2[1:])
    s = f2_inv(n2[0])
    return f12_mul(f12_conjugate(a), tuple(f2_mul(x, s) for x in co))


# the library's tower order: c0.c0, c0.c1, c0.c2, c1.c0, c1.c1, c1.c2  <->  a_0, a_2, a_4, a_1, a_3, a_5
_ORDER = (0, 2, 4, 1, 3, 5)


def to_tower(a):
    return tuple(a[i] for i in _ORDER)


def from_tower(t):
    a = [None] * 6
    for pos, i in enumerate(_ORDER):
        a[i] = t[pos]
    return tuple(a)


def fq6_embed(c):
    """(c0, c1, c2) of Fq6 = Fq2[v]/(v^3 - xi) as an element of Fq12 (v = w^2)"""
    return (c[0], F2_ZERO, c[1], F2_ZERO, c[2], F2_ZERO)


def fq6_project(a):
    assert all(a[i] == F2_ZERO for i in (1, 3, 5))
    return (a[0], a[2], a[4])


def line_034(c0, c3, c4):
    """the sparse element of mul_by_034: c0 + (c3 + c4 v) w = c0 + c3 w + c4 w^3"""
    return (c0, c3, F2_ZERO, c4, F2_ZERO, F2_ZERO)


# ---------------------------------------------------------------- the 384-byte GT format: twelve Montgomery Fq, 4 u64 limbs each
def gt_to_words(a) -> list[int]:
    out = []
    for c in to_tower(a):
        for x in c:
            out += M.to_limbs(M.to_mont(x, Q))
    return out


def gt_from_words(words):
    words = [int(v) for v in words]
    assert len(words) == 48
    fq = [M.from_mont(M.from_limbs(words[4 * i:4 * i + 4]), Q) for i in range(12)]
    return from_tower(tuple((fq[2 * i], fq[2 * i + 1]) for i in range(6)))


# ---------------------------------------------------------------- the pairing
F2 = M.FQ2_OPS
TWIST_FROB_X = f2_pow(XI, (Q - 1) // 3)
TWIST_FROB_Y = f2_pow(XI, (Q - 1) // 2)


def twist_frobenius(p):
    """the q-power Frobenius of E(Fq12) carried to the twist: (x, y) -> (conj(x) xi^((q-1)/3), conj(y) xi^((q-1)/2))"""
    return (f2_mul(f2_conj(p[0]), TWIST_FROB_X), f2_mul(f2_conj(p[1]), TWIST_FROB_Y))


def _line(t, s, p):
    """The line through the twist points t and s (the tangent if they are equal) at the G1 point p, through the untwist
    (x', y') -> (x' w^2, y' w^3):  y_P - lambda x_P w + (lambda x_t - y_t) w^3."""
    if t == s:
        lam = f2_mul(f2_mul((3, 0), f2_mul(t[0], t[0])), f2_inv(f2_add(t[1], t[1])))
    else:
        assert t[0] != s[0], "vertical line: not met for points of order r"
        lam = f2_mul(f2_sub(s[1], t[1]), f2_inv(f2_sub(s[0], t[0])))
    a1 = f2_neg((lam[0] * p[0] % Q, lam[1] * p[0] % Q))
    a3 = f2_sub(f2_mul(lam, t[0]), t[1])
    return ((p[1] % Q, 0), a1, F2_ZERO, a3, F2_ZERO, F2_ZERO)


def miller_loop(p, q):
    """p: affine G1 point (x, y) of ints or None; q: affine G2 point on the twist or None.  A pair with a point at infinity gives one."""
    if p is None or q is None:
        return ONE
    f, t = ONE, q
    for bit in bin(ATE_LOOP)[3:]:
        f = f12_mul(f12_sqr(f), _line(t, t, p))
        t = M.ec_add(F2, t, t)
        if bit == "1":
            f = f12_mul(f, _line(t, q, p))
            t = M.ec_add(F2, t, q)
    q1 = twist_frobenius(q)
    q2 = M.ec_neg(F2, twist_frobenius(q1))
    f = f12_mul(f, _line(t, q1, p))
    t = M.ec_add(F2, t, q1)
    return f12_mul(f, _line(t, q2, p))


def final_exponentiation(f):
    return f12_pow(f, FINAL_EXPONENT)


def pairing(p, q):
    return final_exponentiation(miller_loop(p, q))


def pairing_product(pairs):
    f = ONE
    for p, q in pairs:
        f = f12_mul(f, miller_loop(p, q))
    return final_exponentiation(f)
