"""Edge operands for the field and group-law primitives of csrc/field.hpp, fieldu.hpp and curveu.hpp, with their big-int expectations.

TEST INFRASTRUCTURE, plain Python, no GPU.  One seeded generator that both legs import: tests/test_field_edges_host.py (the table and
the reference, through the host-compiled hooks where one exists) and tests/test_gpu_field_edges.py (the same table through
mi355zk_selftest_dev_op, one primitive per lane on the device).

Every op of `enum mi355zk_devop` (include/mi355zk.h) has an `Op` here (a test compares the two sets).  An Op yields named cases
(class name, input words) that lie INSIDE the contract written next to the primitive -- the contract is restated as assertions in
`Op.expect`, which also computes the big-int reference -- and `Op.verify` checks a result against it.  An operand outside the contract
is a generator bug, never a test case: nothing is filtered after generation.

Words: an Fp element is 8 x 32-bit words of the integer; a U-form element 9 limbs of 29 bits held in u32 (value = sum l[i] 2^(29 i)),
"N-form" meaning l[0..7] < 2^29.
"""
from __future__ import annotations

import random

import bn254_model as M

N_RANDOM = 4096          # uniform random cases per op on top of the named classes
N_RANDOM_GROUPS = 1024   # ... per lane-group op (each case fills 4 or 2 lanes)
SEED = 0x5EED_ED6E
MASK29, MASK32 = (1 << 29) - 1, (1 << 32) - 1
MODS = {0: M.Q, 1: M.R_ORDER}
RU = 1 << 261            # the Montgomery radix of the U-form
CHAIN = 0x100            # MI355ZK_DEVOP_CHAIN


# ------------------------------------------------------------------------------------------------ words <-> integers
def w32(v, n=8):
    assert 0 <= v < 1 << (32 * n)
    return [(v >> (32 * i)) & MASK32 for i in range(n)]


def v32(w):
    return sum(int(x) << (32 * i) for i, x in enumerate(w))


def l29(v):
    """the N-form limb vector of v (unique): limbs 0..7 < 2^29, limb 8 the rest"""
    assert 0 <= v < 1 << (232 + 32)
    return [(v >> (29 * i)) & MASK29 for i in range(8)] + [v >> 232]


def v29(l):
    return sum(int(x) << (29 * i) for i, x in enumerate(l))


def is_n(l):
    return all(0 <= x < 1 << 29 for x in l[:8]) and 0 <= l[8] < 1 << 32


def redundant(v, extra_bits, rnd):
    """a non-normalised limb vector of the same integer: limbs 0..7 up to 2^(29 + extra_bits) (as tests/test_uform_host.py makes them)"""
    l = l29(v)
    for i in range(8):
        if l[i + 1] > 0:
            take = rnd.randrange(0, min(l[i + 1], (1 << extra_bits) - 1) + 1)
            l[i + 1] -= take
            l[i] += take << 29
    assert v29(l) == v
    return l


def redundant_max(v, extra_bits):
    """the same with every borrow at its maximum: limbs 0..7 as large as the value allows below 2^(29 + extra_bits)"""
    l = l29(v)
    for i in range(8):
        take = min(l[i + 1], (1 << extra_bits) - 1)
        l[i + 1] -= take
        l[i] += take << 29
    assert v29(l) == v
    return l


def hexw(words):
    return "[" + " ".join("%08x" % int(x) for x in words) + "]"


# ------------------------------------------------------------------------------------------------ value classes
def fp_values(p):
    """named canonical values (< p)"""
    R = (1 << 256) % p
    out = [("0", 0), ("1", 1), ("2", 2), ("p-1", p - 1), ("p-2", p - 2), ("(p-1)/2", (p - 1) // 2), ("(p+1)/2", (p + 1) // 2),
           ("R", R), ("R^2", R * R % p), ("-R", p - R)]
    for k in range(32, 254, 32):
        out += [("2^%d" % k, 1 << k), ("2^%d-1" % k, (1 << k) - 1)]
    for k in range(29, 254, 29):
        out += [("2^%d" % k, 1 << k), ("2^%d-1" % k, (1 << k) - 1)]
    for i in range(8):
        for d in (1, -1):
            v = p + d * (1 << (32 * i))
            if 0 <= v < p:
                out.append(("p%+d*2^%d" % (d, 32 * i), v))
    alt_a = sum(MASK32 << (64 * i) for i in range(4))          # ffffffff 00000000 ... from limb 0
    alt_b = alt_a << 32 & ((1 << 256) - 1)
    for name, v in (("alt_ff00", alt_a), ("alt_00ff", alt_b)):
        while v >= p:                                              # the largest such pattern below p: clear top limbs
            top = v.bit_length() - 1
            v &= (1 << (top // 32 * 32)) - 1
        out.append((name, v))
    # all-ones limbs below the top limb: the largest value below p whose seven low limbs are ffffffff
    out.append(("low_limbs_ff", ((p >> 224) - 1 << 224) | ((1 << 224) - 1)))
    for n, v in out:
        assert 0 <= v < p, n
    return out


def u_values(p, kmax):
    """named values for a lazy U-form operand bounded by value <= kmax * p"""
    out = []
    for name, v in fp_values(p):
        out.append((name, v))
    for j in range(1, kmax):
        out += [("%dp-1" % j, j * p - 1), ("%dp" % j, j * p), ("%dp+1" % j, j * p + 1), ("(p-1)+%dp" % j, p - 1 + j * p)]
    out.append(("%dp-1" % kmax, kmax * p - 1))
    return out


# ------------------------------------------------------------------------------------------------ the Fp product's column schedule
def fp_mul_schedule():
    """the (kind, i, j) multiply-accumulates of mont_mul_gfx950.inc (tools/gen_mont_mul.py), column by column, in issue order"""
    cols = []
    for k in range(16):
        lo, hi = max(0, k - 7), min(k, 7)
        seq = [("ab", i, k - i) for i in range(lo, hi + 1)]
        if k < 8:
            seq += [("mp", i, k - i) for i in range(0, k)] + [("m", k, 0)]
        else:
            seq += [("mp", i, k - i) for i in range(k - 7, 8)]
        cols.append(seq)
    return cols


FP_MUL_SCHEDULE = fp_mul_schedule()
FP_MUL_MACS = [(k, n) for k, seq in enumerate(FP_MUL_SCHEDULE) for n in range(len(seq))]   # 128 (column, position) pairs
assert len(FP_MUL_MACS) == 128


def fp_mul_columns(a, b, p, drop=None):
    """Python model of the device product: 64-bit accumulator + third word per column.  Returns (r before reduce_once, m[0..7],
    third word per column, the set of (column, position) whose v_addc_co_u32 saw a carry).  drop = (column, position): that addc is
    missing (the mutation a careless edit of the generated file makes)."""
    A, B, P = w32(a), w32(b), w32(p)
    inv = (-pow(p, -1, 1 << 32)) & MASK32
    m, r, third, carried = [0] * 8, [0] * 8, [], set()
    acc = c2 = 0
    for k, seq in enumerate(FP_MUL_SCHEDULE):
        for n, (kind, i, j) in enumerate(seq):
            if kind == "m":
                m[i] = (acc & MASK32) * inv & MASK32
            x, y = (A[i], B[j]) if kind == "ab" else (m[i], P[j])
            acc += x * y
            if acc >> 64:
                acc &= (1 << 64) - 1
                carried.add((k, n))
                if drop != (k, n):
                    c2 += 1
        if k >= 8:
            r[k - 8] = acc & MASK32
        third.append(c2)
        acc = (acc >> 32) | (c2 << 32)
        c2 = 0
    return v32(r), m, third, carried


def _with_m(p, m_target, rnd, a_pool):
    """(a, b) < p whose product has the given Montgomery quotient m = -a b / p mod 2^256 (its 32-bit digits are the m[k] of the schedule)"""
    for a in a_pool:
        if a % 2 == 0:
            continue
        b = (-m_target * p) * pow(a, -1, 1 << 256) % (1 << 256)
        if b < p:
            return a, b
    while True:
        a = rnd.randrange(1, p) | 1
        b = (-m_target * p) * pow(a, -1, 1 << 256) % (1 << 256)
        if a < p and b < p:
            return a, b


def fp_mul_directed(p, rnd):
    """operand pairs chosen with the column model: every m[k] at 0 and at ffffffff, the third word of every column at 0 and at the
    largest count a search finds, the value before reduce_once on both sides of p"""
    ones = (1 << 256) - 1
    big = [v for _, v in fp_values(p) if v > p >> 1]
    out = [("m=0:2^128*x", (rnd.randrange(1, 1 << 125) << 128, rnd.randrange(1, 1 << 125) << 128)),
           ("m=all_ones", _with_m(p, ones, rnd, big))]
    for k in range(8):
        base = rnd.getrandbits(256)
        out.append(("m[%d]=0" % k, _with_m(p, base & ~(MASK32 << (32 * k)), rnd, big)))
        out.append(("m[%d]=ffffffff" % k, _with_m(p, base | (MASK32 << (32 * k)), rnd, big)))
        out.append(("m[%d]=ffffffff,rest=0" % k, _with_m(p, MASK32 << (32 * k), rnd, [])))
    # third word: hill climb on the column's carry count from large operands; all carries of a column need large limbs on its diagonal
    hi = [p - 1, p - 2, ((p >> 224) - 1 << 224) | ((1 << 224) - 1), (p >> 224 << 224) - 1]
    for a in hi:
        for b in hi:
            out.append(("large*large", (a, b)))
    for k in range(15):
        best, best_ab = -1, None
        for trial in range(60):
            a, b = rnd.choice(hi), rnd.choice(hi)
            for w in range(8):                                    # limbs off the column's diagonals random, on them at the maximum
                if not (max(0, k - 7) <= w <= min(k, 7)):
                    a = a & ~(MASK32 << (32 * w)) | (rnd.getrandbits(32) << (32 * w))
                    b = b & ~(MASK32 << (32 * w)) | (rnd.getrandbits(32) << (32 * w))
            a, b = a % p, b % p
            t = fp_mul_columns(a, b, p)[2][k]
            if t > best:
                best, best_ab = t, (a, b)
        out.append(("third[%d]=max_found" % k, best_ab))
        out.append(("third[%d]=0" % k, (rnd.randrange(1 << (32 * max(1, k - 6))) % p, 1)))
    # both sides of p before the final subtraction
    lo_side = hi_side = None
    while lo_side is None or hi_side is None:
        a, b = rnd.randrange(p), rnd.randrange(p)
        if fp_mul_columns(a, b, p)[0] >= p:
            hi_side = (a, b)
        else:
            lo_side = (a, b)
    out += [("pre_reduce>=p", hi_side), ("pre_reduce<p", lo_side)]
    for n, (a, b) in out:
        assert 0 <= a < p and 0 <= b < p, n
    return out


# ------------------------------------------------------------------------------------------------ ops
class Op:
    """name: the enum name without its prefix.  fields: the `which` values it exists for.  group: lanes per case."""

    def __init__(self, name, in_words, out_words, fields=(0, 1), group=1, chain=False, host=None):
        self.name, self.in_words, self.out_words, self.fields, self.group, self.chain, self.host = name, in_words, out_words, fields, group, chain, host

    def cases(self, which):      # -> list of (class name, input words)
        raise NotImplementedError

    def expect(self, which, inw):   # asserts the contract on the operands, returns the reference
        raise NotImplementedError

    def verify(self, which, inw, outw, exp):   # raises AssertionError
        raise NotImplementedError

    def table(self, which):
        key = (self.name, which)
        if key not in _TABLES:
            rows = self.cases(which)
            for cls, inw in rows:
                assert len(inw) == self.in_words and all(0 <= int(x) <= MASK32 for x in inw), (self.name, cls)
            _TABLES[key] = rows
        return _TABLES[key]

    def describe(self, which, cls, inw):
        return "op %s, field %s, class %s, operands %s" % (self.name, ("Fq", "Fr")[which], cls, hexw(inw))


_TABLES: dict = {}


def _rng(name, which):
    return random.Random("%x/%s/%d" % (SEED, name, which))


# ---- Fp (8 x 32, canonical)
class FpOp(Op):
    """contract (field.hpp): operands canonical, a, b < p; reduce_once: a < 2p.  Result canonical, equal to the big-int one limb for limb.
    mul / sqr are Montgomery: a b 2^-256."""

    def __init__(self, name, arity, fn):
        super().__init__("FP_" + name, 8 * arity, 8)
        self.arity, self.fn = arity, fn

    def cases(self, which):
        p, rnd, nm = MODS[which], _rng(self.name, which), self.name[3:]
        vals = fp_values(p)
        rows = []
        if nm == "REDUCE_ONCE":
            for n, v in vals:
                rows += [(n, [v]), (n + "+p", [v + p])]
            rows += [("random<2p", [rnd.randrange(2 * p)]) for _ in range(N_RANDOM)]
        elif self.arity == 1:
            rows += [(n, [v]) for n, v in vals]
            rows += [("random", [rnd.randrange(p)]) for _ in range(N_RANDOM)]
        else:
            rows += [("%s , %s" % (na, nb), [a, b]) for na, a in vals for nb, b in vals]
            rinv = pow(1 << 256, -1, p)
            for n, a in vals:
                rows += [("a+b=p-1", [a, (p - 1 - a) % p]), ("a+b=p", [a, (p - a) % p]), ("a-b=0", [a, a]), ("a-b=-1", [a, (a + 1) % p])]
                if a + 1 < p and a >= 1:
                    rows.append(("a+b=p+1", [a + 1, p - a]))
                if a:
                    for t, tn in ((0, "0"), (1, "1"), (p - 1, "p-1")):
                        rows.append(("a*b/R=" + tn, [a, t * pow(a * rinv, -1, p) % p]))
            if nm == "MUL":
                rows += [(n, list(ab)) for n, ab in fp_mul_directed(p, rnd)]
            rows += [("random", [rnd.randrange(p), rnd.randrange(p)]) for _ in range(N_RANDOM)]
        return [(cls, sum((w32(v) for v in ops), [])) for cls, ops in rows]

    def expect(self, which, inw):
        p = MODS[which]
        ops = [v32(inw[8 * i:8 * i + 8]) for i in range(self.arity)]
        for v in ops:
            assert v < (2 * p if self.name == "FP_REDUCE_ONCE" else p), "operand outside the contract"
        return self.fn(p, *ops)

    def verify(self, which, inw, outw, exp):
        assert v32(outw) == exp, "got %s, want %s" % (hexw(outw), hexw(w32(exp)))


def _rinv(p):
    return pow(1 << 256, -1, p)


FP_OPS = [
    FpOp("MUL", 2, lambda p, a, b: a * b * _rinv(p) % p),
    FpOp("SQR", 1, lambda p, a: a * a * _rinv(p) % p),
    FpOp("ADD", 2, lambda p, a, b: (a + b) % p),
    FpOp("SUB", 2, lambda p, a, b: (a - b) % p),
    FpOp("DBL", 1, lambda p, a: 2 * a % p),
    FpOp("NEG", 1, lambda p, a: -a % p),
    FpOp("REDUCE_ONCE", 1, lambda p, a: a % p),
    FpOp("INV", 1, lambda p, a: pow(a * _rinv(p), -1, p) * (1 << 256) % p if a else 0),   # Montgomery in and out; inv(0) = 0 (field.hpp)
]


# ---- Fq2 (canonical pairs)
class Fq2Op(Op):
    def __init__(self, name, arity, fn):
        super().__init__("FQ2_" + name, 16 * arity, 16, fields=(0,))
        self.arity, self.fn = arity, fn

    def cases(self, which):
        p, rnd = M.Q, _rng(self.name, which)
        vals = fp_values(p)
        small = [v for v in vals if v[0] in ("0", "1", "p-1", "(p+1)/2", "R", "-R", "2^224-1", "alt_ff00", "low_limbs_ff")]
        els = [("(%s,%s)" % (n0, n1), (v0, v1)) for n0, v0 in small for n1, v1 in small]
        rows = []
        if self.arity == 1:
            rows += els + [("(%s,0)" % n, (v, 0)) for n, v in vals] + [("(0,%s)" % n, (0, v)) for n, v in vals]
            rows += [("c0=c1", (v, v)) for _, v in vals] + [("c0=-c1", (v, -v % p)) for _, v in vals]     # sqr: a0 - a1 = 0 / a0 + a1 = p
            rows = [(n, [e]) for n, e in rows]
            rows += [("random", [(rnd.randrange(p), rnd.randrange(p))]) for _ in range(N_RANDOM)]
        else:
            rows += [("%s , %s" % (na, nb), [a, b]) for na, a in els[::3] for nb, b in els[::2]]
            for n, a in els:
                rows += [("a+b=0", [a, M.f2_neg(a)]), ("a-b=0", [a, a]), ("a+b=(p-1,p-1)", [a, M.f2_sub((p - 1, p - 1), a)])]
                if a != (0, 0):
                    ai = M.f2_inv(M.f2_mul(a, (_rinv(p), 0)))
                    for t in ((1, 0), (p - 1, 0), (0, 1), (0, p - 1)):
                        rows.append(("a*b/R=%s" % (t,), [a, M.f2_mul(t, ai)]))
            rows += [("random", [(rnd.randrange(p), rnd.randrange(p)), (rnd.randrange(p), rnd.randrange(p))]) for _ in range(N_RANDOM)]
        return [(cls, sum((w32(e[0]) + w32(e[1]) for e in ops), [])) for cls, ops in rows]

    def expect(self, which, inw):
        ops = [(v32(inw[16 * i:16 * i + 8]), v32(inw[16 * i + 8:16 * i + 16])) for i in range(self.arity)]
        for e in ops:
            assert e[0] < M.Q and e[1] < M.Q, "operand outside the contract"
        return self.fn(*ops)

    def verify(self, which, inw, outw, exp):
        got = (v32(outw[:8]), v32(outw[8:]))
        assert got == exp, "got %s, want %s" % (hexw(outw), hexw(w32(exp[0]) + w32(exp[1])))


def _f2_scale(a, s):
    return (a[0] * s % M.Q, a[1] * s % M.Q)


FQ2_OPS = [
    Fq2Op("MUL", 2, lambda a, b: _f2_scale(M.f2_mul(a, b), _rinv(M.Q))),
    Fq2Op("SQR", 1, lambda a: _f2_scale(M.f2_mul(a, a), _rinv(M.Q))),
    Fq2Op("INV", 1, lambda a: _f2_scale(M.f2_inv(a), (1 << 512) % M.Q) if a != (0, 0) else (0, 0)),
    Fq2Op("ADD", 2, M.f2_add),
    Fq2Op("SUB", 2, M.f2_sub),
    Fq2Op("NEG", 1, M.f2_neg),
]


# ---- FpU (9 x 29, lazy)
def mont_u(p, prods):
    """the exact Montgomery result of u_mul / u_sqr / u_mul2..4: (T + m p) / 2^261 with m = -T / p mod 2^261, T the sum of the products"""
    T = sum(a * b for a, b in prods)
    m = -T * pow(p, -1, RU) % RU
    assert (T + m * p) % RU == 0
    return (T + m * p) >> 261


def shoup_model(p, a, w):
    """u_mul_shoup as fieldu.hpp computes it: q from columns 7 .. 16 of a * wq (the low columns dropped), r = a w - q p mod 2^261.
    This RESTATES the implementation's truncated quotient: the `exact` expectation built on it pins the algorithm (host = device = this), it is
    not an independent reference.  The independent checks of u_mul_shoup are the residue (a w mod p), the bound (< 2p) and limb 8 < 2^23."""
    wq = l29((w << 261) // p)
    T = sum(a[i] * wq[j] << (29 * (i + j - 7)) for i in range(9) for j in range(9) if i + j >= 7)
    q = T >> 58
    return (v29(a) * w - q * p) % RU, v29(wq)


class UOp(Op):
    """One FpU primitive.  `gen(p, rnd)` yields (class, list of limb vectors / Fp words); `ref(p, operands)` asserts the contract and returns
    a dict: exact (the exact integer result, if the op determines one), mod (the residue), bound (value < bound), limb_bound (limbs 0..7),
    std (canonical 8 x 32 result) or flag."""

    def __init__(self, name, shape, gen, ref, host=None, fields=(0, 1)):
        kind = ref.__annotations__["return"].strip("'\"")     # what the op returns: a U-form element, a canonical one, a flag, two U-form elements
        super().__init__("U_" + name, sum(shape), {"u": 9, "s": 8, "f": 1, "uu": 18}[kind], fields=fields, chain=True, host=host)
        self.shape, self.gen, self.ref, self.kind = shape, gen, ref, kind

    def cases(self, which):
        return [(cls, sum((list(o) for o in ops), [])) for cls, ops in self.gen(MODS[which], _rng(self.name, which))]

    def split(self, inw):
        out, o = [], 0
        for n in self.shape:
            out.append([int(x) for x in inw[o:o + n]])
            o += n
        return out

    def expect(self, which, inw):
        return self.ref(MODS[which], self.split(inw))

    def verify(self, which, inw, outw, exp):
        p = MODS[which]
        outw = [int(x) for x in outw]
        if self.kind == "s":
            assert v32(outw) == exp["std"], "got %s, want %s" % (hexw(outw), hexw(w32(exp["std"])))
        elif self.kind == "f":
            assert outw[0] == exp["flag"], "got %d, want %d" % (outw[0], exp["flag"])
        else:
            check_u(p, outw[:9], exp)
            if self.kind == "uu":
                assert v29(outw[9:]) == exp["wq"] and is_n(outw[9:]) and outw[17] < 1 << 29, "quotient of the constant: got %s" % hexw(outw[9:])


def check_u(p, l, exp):
    v = v29(l)
    if "limbs" in exp:
        assert l == exp["limbs"], "got %s, want %s" % (hexw(l), hexw(exp["limbs"]))
        return
    if exp.get("n_form", True):
        assert is_n(l), "not N-form: %s" % hexw(l)
    if "exact" in exp:
        assert v == exp["exact"], "got value %x (%s), want %x" % (v, hexw(l), exp["exact"])
    assert v % p == exp["mod"], "value %x (%s) is not congruent to %x" % (v, hexw(l), exp["mod"])
    assert v < exp["bound"], "value %x (%s) is not below the stated bound %x" % (v, hexw(l), exp["bound"])
    if "top_bound" in exp:
        assert l[8] < exp["top_bound"], "limb 8 of %s is not below %x" % (hexw(l), exp["top_bound"])


def _lazy(p, rnd, kmax, extra_bits, n_random):
    """operands with value <= kmax p - 1 and limbs 0..7 < 2^(29 + extra_bits): named values, each as N-form and as redundant twins"""
    rows = []
    for n, v in u_values(p, kmax):
        rows.append((n, l29(v)))
        if extra_bits:
            rows.append((n + "~max_limbs", redundant_max(v, extra_bits)))
            rows.append((n + "~redundant", redundant(v, extra_bits, rnd)))
    for _ in range(n_random):
        v = rnd.randrange(kmax * p)
        rows.append(("random", redundant(v, extra_bits, rnd) if extra_bits and rnd.random() < 0.5 else l29(v)))
    return rows


def _pairs(named_a, named_b, rand_a, rand_b, rnd):
    """all named x named pairs of two operand lists + the random ones paired up"""
    rows = [("%s , %s" % (na, nb), [a, b]) for na, a in named_a for nb, b in named_b]
    rows += [("random", [a, b]) for (_, a), (_, b) in zip(rand_a, rand_b)]
    return rows


def _split_named(rows):
    return [r for r in rows if r[0] != "random"], [r for r in rows if r[0] == "random"]


def _thin(rows, k):
    return rows[::k]


def gen_from_std(p, rnd):
    return [(n, [w32(v)]) for n, v in fp_values(p)] + [("random", [w32(rnd.randrange(p))]) for _ in range(N_RANDOM)]


def ref_from_std(p, ops) -> "u":
    v = v32(ops[0])
    assert v < p                                             # callers re-pack canonical memory-format values
    return {"limbs": l29(v)}


def gen_carry(p, rnd):
    # contract (u_carry): every l[i] + carry-in < 2^32, "limbs < 2^32 - 2^4"
    top = (1 << 32) - (1 << 4) - 1
    rows = [("all_limbs_max", [[top] * 9]), ("zero", [[0] * 9]), ("limbs_2^29", [[1 << 29] * 9]), ("limbs_2^29-1", [[MASK29] * 9])]
    for i in range(9):
        rows.append(("limb%d_max" % i, [[top if j == i else 0 for j in range(9)]]))
        rows.append(("ripple_from_%d" % i, [[0] * i + [1 << 29] + [MASK29] * (8 - i)]))
    rows += [(n, [l]) for n, l in _lazy(p, rnd, 32, 2, 0)]
    rows += [("random_limbs", [[rnd.randrange(top + 1) for _ in range(9)]]) for _ in range(N_RANDOM)]
    return rows


def ref_carry(p, ops) -> "u":
    a = ops[0]
    assert all(x < (1 << 32) - (1 << 4) for x in a)
    v = v29(a)
    assert v < 1 << 264                                      # limb 8 + carry-in < 2^32
    return {"limbs": l29(v)}


def gen_to_std(kmax):
    def gen(p, rnd):
        rows = [(n, [l]) for n, l in _lazy(p, rnd, kmax, 0, N_RANDOM)]
        rows += [("%dp%+d" % (k, d), [l29(k * p + d)]) for k in range(kmax + 1) for d in (-1, 0, 1) if 0 <= k * p + d < kmax * p]
        return rows
    return gen


def ref_to_std(kmax):
    def ref(p, ops) -> "s":
        a = ops[0]
        assert is_n(a) and v29(a) < kmax * p                  # "N-form value < 2p" / "< 32p" (then a.l[8] < 2^28)
        return {"std": v29(a) % p}
    return ref


def gen_add(p, rnd):
    named, rand = _split_named(_lazy(p, rnd, 8, 2, N_RANDOM))
    rows = _pairs(_thin(named, 7), _thin(named, 5), rand, rand[::-1], rnd)
    rows.append(("limbs_2^31-1 , limbs_2^31", [[(1 << 31) - 1] * 9, [1 << 31] * 9]))
    return rows


def ref_add(p, ops) -> "u":
    a, b = ops
    assert all(x + y < 1 << 32 for x, y in zip(a, b))         # no normalisation, no wrap
    return {"limbs": [x + y for x, y in zip(a, b)]}


def gen_dbl(p, rnd):
    return [(n, [l]) for n, l in _lazy(p, rnd, 8, 2, N_RANDOM)] + [("limbs_2^31-1", [[(1 << 31) - 1] * 9])]


def ref_dbl(p, ops) -> "u":
    assert all(x < 1 << 31 for x in ops[0])
    return {"limbs": [2 * x for x in ops[0]]}


def gen_sub(K, S):
    def gen(p, rnd):
        # b: limbs 0..7 < S 2^29, value <= K p.   a: limbs 0..7 < 2^32 - (S + 1) 2^29 - 2^4; the kernels' minuends are below 32p
        eb = {1: 0, 2: 1, 3: 2}[S]
        lim_b = S << 29
        b_named = []
        for n, v in u_values(p, K) + [("%dp" % K, K * p)]:
            b_named.append((n, l29(v)))
            if eb:
                for nm, l in ((n + "~max_limbs", redundant_max(v, eb)), (n + "~redundant", redundant(v, eb, rnd))):
                    l = [min(x, lim_b - 1) if i < 8 else x for i, x in enumerate(l)]
                    if v29(l) == v:
                        b_named.append((nm, l))
        a_cap = (1 << 32) - ((S + 1) << 29) - (1 << 4) - 1
        a_named = [(n, l29(v)) for n, v in u_values(p, 2)] + [("0", [0] * 9), ("31p", l29(31 * p)), ("limbs_max", [a_cap] * 8 + [1 << 20]),
                                                                ("limbs_max,top0", [a_cap] * 8 + [0])]
        rows = _pairs(_thin(a_named, 3), b_named, [], [], rnd)
        for n, lb in b_named:
            v = v29(lb)
            rows += [("a-b=0", [l29(v), lb]), ("a-b=-1", [l29(v - 1), lb] if v else [l29(0), lb]), ("a=0", [[0] * 9, lb])]
        for _ in range(N_RANDOM):
            vb = rnd.randrange(K * p + 1)
            lb = redundant(vb, eb, rnd) if eb and rnd.random() < 0.5 else l29(vb)
            lb = lb if all(x < lim_b for x in lb[:8]) else l29(vb)
            va = rnd.randrange(32 * p)
            la = redundant(va, 1, rnd) if rnd.random() < 0.5 else l29(va)
            rows.append(("random", [la, lb]))
        return rows
    return gen


def ref_sub(K, S):
    def ref(p, ops) -> "u":
        a, b = ops
        assert all(x < S << 29 for x in b[:8]) and v29(b) <= K * p
        assert all(x < (1 << 32) - ((S + 1) << 29) - (1 << 4) for x in a[:8])
        v = v29(a) + K * p - v29(b)
        assert 0 <= v < 1 << 264
        return {"limbs": l29(v)}                             # N-form of the exact value: the result is determined
    return ref


def _mul_operands(p, rnd, n_random):
    """u_mul: max_limb(a) max_limb(b) < 2^60.5 -- both below 2^30, or one N-form and the other below 2^31.5; values up to 10p"""
    a30 = _lazy(p, rnd, 10, 1, n_random)
    top = l29(10 * p - 1)[8]
    a30 += [("limbs_2^30-1,top_10p", [(1 << 30) - 1] * 8 + [top]), ("limbs_2^30-1_all", [(1 << 30) - 1] * 9)]
    return a30


def gen_mul(p, rnd):
    rows30 = _mul_operands(p, rnd, N_RANDOM)
    named, rand = _split_named(rows30)
    rows = _pairs(_thin(named, 5), _thin(named, 3), rand, rand[::-1], rnd)
    rows.append(("limbs_2^30-1_all , same", [[(1 << 30) - 1] * 9] * 2))
    # one N-form, the other with limbs up to 2^31.5 (4X in jacu_double: limbs < 2^31)
    wide = int(2 ** 31.5) - 1
    nn = [l for _, l in _thin(_lazy(p, rnd, 2, 0, 0), 4)] + [[MASK29] * 9]
    for l in nn:
        rows.append(("N-form , limbs_2^31.5", [l, [wide] * 8 + [wide]]))
        rows.append(("limbs_4x(6p-1) , N-form", [[4 * x for x in l29(6 * p - 1)], l]))
    ru = pow(RU, 1, p)
    for n, la in _thin(named, 9):
        a = v29(la)
        if a % p:
            for t, tn in ((0, "0"), (1, "1"), (p - 1, "p-1")):
                rows.append(("a*b/R'=" + tn, [la, l29(t * ru * pow(a, -1, p) % p)]))
    return rows


def _ref_products(p, pairs):
    T = sum(v29(a) * v29(b) for a, b in pairs)
    exact = mont_u(p, [(v29(a), v29(b)) for a, b in pairs])
    assert exact < 1 << 264
    return {"exact": exact, "mod": T * pow(RU, -1, p) % p, "bound": T // RU + p + 1, "n_form": True}


def ref_mul(p, ops) -> "u":
    a, b = ops
    assert max(a) * max(b) < 2 ** 60.5
    return _ref_products(p, [(a, b)])


def gen_sqr(p, rnd):
    return [(n, [l]) for n, l in _lazy(p, rnd, 10, 0, N_RANDOM)] + [("limbs_2^29-1_all", [[MASK29] * 9])]


def ref_sqr(p, ops) -> "u":
    assert is_n(ops[0]) and ops[0][8] < 1 << 29              # "a N-form (limbs < 2^29)"
    return _ref_products(p, [(ops[0], ops[0])])


def gen_muln(n):
    def gen(p, rnd):
        named, _ = _split_named(_lazy(p, rnd, 10, 0, 0))
        named.append(("limbs_2^29-1_all", [MASK29] * 9))
        rows = [("all " + nm, [l] * (2 * n)) for nm, l in named]
        for _ in range(300):
            pick = [rnd.choice(named) for _ in range(2 * n)]
            rows.append(("mixed named", [l for _, l in pick]))
        # a b + c d == 0: the second product cancels the first (c = a, d = k p - b)
        for nm, l in _thin(named, 3):
            v = v29(l) % p
            ops = [l, l29(v), l, l29(p - v if v else 0)] + [l29(0), l] * (n - 2)
            rows.append(("sum==0 mod p", ops))
        rows += [("random", [l29(rnd.randrange(10 * p)) for _ in range(2 * n)]) for _ in range(N_RANDOM)]
        return rows
    return gen


def ref_muln(n):
    def ref(p, ops) -> "u":
        assert len(ops) == 2 * n and all(is_n(o) and o[8] < 1 << 29 for o in ops)     # "all operands N-form"
        return _ref_products(p, [(ops[2 * i], ops[2 * i + 1]) for i in range(n)])
    return ref


def gen_shoup(p, rnd):
    # a: limbs < 2^31, value < 160p;  w canonical.  The estimate q is short of floor(a w / p) by at most one for a < 160p: search for those
    consts = [v for _, v in fp_values(p)]
    a_named = _lazy(p, rnd, 160, 0, 0)[::6] + [("160p-1~max_limbs", redundant_max(160 * p - 1, 2)), ("160p-1~redundant", redundant(160 * p - 1, 2, rnd)),
                                              ("(p-1)~max_limbs", redundant_max(p - 1, 2))]
    rows = [("%s , w=%x.." % (n, w >> 224), [la, w32(w)]) for n, la in a_named for w in consts[::4]]
    rows += [("%s , w=p-1" % n, [la, w32(p - 1)]) for n, la in a_named]
    found = 0
    while found < 64:
        va, w = 160 * p - 1 - rnd.randrange(p), rnd.randrange(p)
        la = redundant(va, 2, rnd)
        if shoup_model(p, la, w)[0] >= p:
            rows.append(("quotient_short_by_1", [la, w32(w)]))
            found += 1
    for _ in range(N_RANDOM):
        va = rnd.randrange(160 * p)
        rows.append(("random", [redundant(va, 2, rnd) if rnd.random() < 0.5 else l29(va), w32(rnd.randrange(p))]))
    return rows


def ref_shoup(p, ops) -> "uu":
    a, ww = ops
    w = v32(ww)
    assert w < p and all(x < 1 << 31 for x in a) and v29(a) < 160 * p
    r, wq = shoup_model(p, a, w)
    assert r % p == v29(a) * w % p and r < 2 * p             # the header's claim, on the model
    return {"mod": v29(a) * w % p, "bound": 2 * p, "top_bound": 1 << 23, "wq": wq, "exact": r}


def gen_is_zero(kmax):
    def gen(p, rnd):
        rows = []
        for k in range(kmax):
            rows += [("%dp" % k, [l29(k * p)]), ("%dp+1" % k, [l29(k * p + 1)])]
            if k:
                rows.append(("%dp-1" % k, [l29(k * p - 1)]))
            for i in range(9):                                    # k p with one limb off: a test on fewer than nine limbs would pass it
                l = l29(k * p)
                l[i] ^= 1
                if is_n(l) and v29(l) < kmax * p:
                    rows.append(("%dp^limb%d" % (k, i), [l]))
        rows.append(("%dp-1" % kmax, [l29(kmax * p - 1)]))
        rows += [(n, [l]) for n, l in _lazy(p, rnd, kmax, 0, N_RANDOM)]
        return rows
    return gen


def ref_is_zero(kmax):
    def ref(p, ops) -> "f":
        assert is_n(ops[0]) and v29(ops[0]) < kmax * p
        return {"flag": int(v29(ops[0]) % p == 0)}
    return ref


U_SUB_KS = [(1, 1), (2, 1), (3, 1), (4, 1), (4, 2), (4, 3), (8, 1), (16, 1)]   # the u_sub<K, S> the device code instantiates (grep csrc)
HOST_U_SUB = {(1, 1), (2, 1), (4, 1), (4, 2), (4, 3), (8, 1)}                 # ... of which mi355zk_selftest_u_sub knows these

U_OPS = [
    UOp("FROM_STD", (8,), gen_from_std, ref_from_std, host="u_pack_in"),
    UOp("CARRY", (9,), gen_carry, ref_carry),
    UOp("TO_STD_LT2P", (9,), gen_to_std(2), ref_to_std(2), host="u_pack_out"),
    UOp("TO_STD_LT32P", (9,), gen_to_std(32), ref_to_std(32), host="u_reduce32"),
    UOp("ADD", (9, 9), gen_add, ref_add),
    UOp("DBL", (9,), gen_dbl, ref_dbl),
] + [UOp("SUB_%d_%d" % ks, (9, 9), gen_sub(*ks), ref_sub(*ks), host=("u_sub", ks) if ks in HOST_U_SUB else None) for ks in U_SUB_KS] + [
    UOp("MUL", (9, 9), gen_mul, ref_mul, host="u_mul"),
    UOp("SQR", (9,), gen_sqr, ref_sqr),
    UOp("MUL2", (9,) * 4, gen_muln(2), ref_muln(2)),
    UOp("MUL3", (9,) * 6, gen_muln(3), ref_muln(3)),
    UOp("MUL4", (9,) * 8, gen_muln(4), ref_muln(4)),
    UOp("MUL_SHOUP", (9, 8), gen_shoup, ref_shoup, host="u_mul_shoup"),
    UOp("IS_ZERO_LT2P", (9,), gen_is_zero(2), ref_is_zero(2)),
    UOp("IS_ZERO_LT8P", (9,), gen_is_zero(8), ref_is_zero(8)),
]


# ---- Fq2U
class F2UOp(Op):
    """f2u_mul<K> / f2u_sqr<K> / f2u_sub<K> (curveu.hpp).  mul: a, b N-form (u_mul2's contract), value(b.c1) <= K p; sqr: a N-form,
    value(a.c1) <= K p; sub: u_sub<K, 1> on both components."""

    def __init__(self, what, K):
        super().__init__("F2U_%s_%d" % (what, K), 18 if what == "SQR" else 36, 18, fields=(0,))
        self.what, self.K = what, K

    def cases(self, which):
        p, rnd, K = M.Q, _rng(self.name, which), self.K
        vb = [(n, l29(v)) for n, v in u_values(p, K) + [("%dp" % K, K * p)]]        # the component bounded by K p
        va = [(n, l29(v)) for n, v in u_values(p, 10)][::3] + [("limbs_2^29-1_all", [MASK29] * 9)]
        rows = []
        r10 = lambda: l29(rnd.randrange(10 * p))     # noqa: E731
        rK = lambda: l29(rnd.randrange(K * p + 1))   # noqa: E731
        if self.what == "SQR":
            rows += [("(%s,%s)" % (n0, n1), [l0, l1]) for n0, l0 in va for n1, l1 in vb]
            rows += [("c0=c1 " + n, [l, l]) for n, l in vb] + [("c0+c1=Kp " + n, [l29(K * p - v29(l)), l]) for n, l in vb]
            rows += [("random", [r10(), rK()]) for _ in range(N_RANDOM)]
        elif self.what == "MUL":
            for n0, l0 in va[::4]:
                for n1, l1 in vb[::3]:
                    rows += [("a=(%s,%s) b=(%s,%s)" % (n0, n0, n0, n1), [l0, l0, l0, l1]), ("a=(%s,0) b=(0,%s)" % (n0, n1), [l0, [0] * 9, [0] * 9, l1]),
                             ("a=(%s,%s) b=(%s,%s)" % (n1, n0, n0, n1), [l1, l0, l0, l1])]
            rows += [("b.c1 " + n, [r10(), r10(), r10(), l]) for n, l in vb]
            rows += [("random", [r10(), r10(), r10(), rK()]) for _ in range(N_RANDOM)]
        else:
            a_cap = (1 << 32) - (2 << 29) - (1 << 4) - 1
            for n1, l1 in vb:
                rows += [("a=b (%s)" % n1, [l1, l1, l1, l1]), ("a=0 b=(%s,%s)" % (n1, n1), [[0] * 9, [0] * 9, l1, l1]),
                         ("a=limbs_max b=(%s,0)" % n1, [[a_cap] * 8 + [0], [a_cap] * 8 + [1 << 20], l1, [0] * 9])]
            rows += [("random", [redundant(rnd.randrange(32 * p), 1, rnd), r10(), rK(), rK()]) for _ in range(N_RANDOM)]
        return [(cls, sum(ops, [])) for cls, ops in rows]

    def expect(self, which, inw):
        p, K = M.Q, self.K
        ops = [[int(x) for x in inw[9 * i:9 * i + 9]] for i in range(len(inw) // 9)]
        ri = pow(RU, -1, p)
        if self.what == "SUB":
            a0, a1, b0, b1 = ops
            return [ref_sub(K, 1)(p, [a0, b0]), ref_sub(K, 1)(p, [a1, b1])]
        for o in ops:
            assert is_n(o) and o[8] < 1 << 29
        if self.what == "MUL":
            a0, a1, b0, b1 = map(v29, ops)
            assert b1 <= K * p
            c0 = _ref_products(p, [(ops[0], ops[2]), (ops[1], l29(K * p - b1))])
            c1 = _ref_products(p, [(ops[0], ops[3]), (ops[1], ops[2])])
            assert c0["mod"] == (a0 * b0 - a1 * b1) * ri % p and c1["mod"] == (a0 * b1 + a1 * b0) * ri % p
            return [c0, c1]
        a0, a1 = map(v29, ops)
        assert a1 <= K * p
        c0 = _ref_products(p, [(l29(a0 + a1), l29(a0 + K * p - a1))])
        c1 = _ref_products(p, [([2 * x for x in ops[0]], ops[1])])
        assert c0["mod"] == (a0 * a0 - a1 * a1) * ri % p and c1["mod"] == 2 * a0 * a1 * ri % p
        return [c0, c1]

    def verify(self, which, inw, outw, exp):
        outw = [int(x) for x in outw]
        check_u(M.Q, outw[:9], exp[0])
        check_u(M.Q, outw[9:], exp[1])


F2U_OPS = [F2UOp("MUL", k) for k in (2, 4, 8)] + [F2UOp("SQR", k) for k in (2, 4, 6, 8)] + [F2UOp("SUB", k) for k in (2, 3, 8)]


# ------------------------------------------------------------------------------------------------ group law
class Grp:
    """G1 (n = 1) or G2 (n = 2 base-field components per coordinate) over bn254_model's affine law"""

    def __init__(self, name, n, F, gen, on_curve):
        self.name, self.n, self.F, self.gen, self.on_curve = name, n, F, gen, on_curve
        self.uw, self.fw = 9 * n, 8 * n          # words of a U-form coordinate / of a canonical coordinate

    def comps(self, e):
        return (e,) if self.n == 1 else tuple(e)

    def el(self, cs):
        return cs[0] if self.n == 1 else tuple(cs)

    def scale(self, e, s):
        return self.el([c * s % M.Q for c in self.comps(e)])

    def neg(self, pt):
        return M.ec_neg(self.F, pt)

    def add(self, a, b):
        return M.ec_add(self.F, a, b)

    def coord_words(self, e):                    # canonical Montgomery (2^256) memory format
        return sum((w32(c * (1 << 256) % M.Q) for c in self.comps(e)), [])


def _f2_sqrt(a):
    q = M.Q
    if a == (0, 0):
        return (0, 0)
    norm = (a[0] * a[0] + a[1] * a[1]) % q
    s = pow(norm, (q + 1) // 4, q)
    if s * s % q != norm:
        return None
    for sg in (s, -s % q):
        h = (a[0] + sg) * pow(2, -1, q) % q
        x0 = pow(h, (q + 1) // 4, q)
        if x0 * x0 % q == h and x0:
            x1 = a[1] * pow(2 * x0, -1, q) % q
            if M.f2_mul((x0, x1), (x0, x1)) == a:
                return (x0, x1)
    return None


def twist_point_outside_subgroup():
    """on the twist, not in the order-r subgroup (as tests/test_g2_subgroup.py builds one: x = (c, 1), y a root of x^3 + b')"""
    for c0 in range(3, 300):
        x = (c0, 1)
        y = _f2_sqrt(M.f2_add(M.f2_mul(M.f2_mul(x, x), x), M.B_G2))
        if y is not None and M.on_curve_g2((x, y)) and M.ec_mul(M.FQ2_OPS, (x, y), M.R_ORDER) is not None:
            return (x, y)
    raise AssertionError("no twist point found")


G1 = Grp("G1", 1, M.FQ_OPS, M.G1_GEN, M.on_curve_g1)
G2 = Grp("G2", 2, M.FQ2_OPS, M.G2_GEN, M.on_curve_g2)
_POOLS: dict = {}


def pool(g):
    """named points: G, 2G, 3G, -G, random multiples, (G2) a twist point outside the subgroup; and 64 more for the random cases"""
    if g.name not in _POOLS:
        rnd = _rng("pool" + g.name, 0)
        G = g.gen
        G2_, G3 = g.add(G, G), g.add(g.add(G, G), G)
        named = [("G", G), ("2G", G2_), ("3G", G3), ("-G", g.neg(G)), ("kG", M.ec_mul(g.F, G, rnd.randrange(M.R_ORDER)))]
        if g.n == 2:
            named.append(("twist_not_subgroup", twist_point_outside_subgroup()))
        more, acc = [], M.ec_mul(g.F, G, rnd.randrange(M.R_ORDER))
        step = M.ec_mul(g.F, G, rnd.randrange(M.R_ORDER))
        for _ in range(64):
            acc = g.add(acc, step)
            more.append(acc)
        for _, pt in named:
            assert g.on_curve(pt)
        _POOLS[g.name] = (named, more)
    return _POOLS[g.name]


def enc_point(g, pt, z, lifts, zz_pow):
    """register form X, Y, ZZ, ZZZ of pt with ZZ = z^2: X, Y carry 2^261, ZZ, ZZZ carry 2^zz_pow (261: register form of the records;
    266: the bucket accumulator); coordinate c (component i) is lifted by lifts[c][i] * p -- a lazy twin inside the invariant
    X < 6p, Y, ZZ, ZZZ < 2p (curveu.hpp).  None: infinity, literal zeros."""
    if pt is None:
        return [0] * (4 * g.uw)
    F, q = g.F, M.Q
    zz = F.mul(z, z)
    zzz = F.mul(zz, z)
    coords = [g.scale(F.mul(pt[0], zz), RU % q), g.scale(F.mul(pt[1], zzz), RU % q), g.scale(zz, (1 << zz_pow) % q), g.scale(zzz, (1 << zz_pow) % q)]
    out = []
    for c, e in enumerate(coords):
        for i, v in enumerate(g.comps(e)):
            j = lifts[c][i]
            assert 0 <= j < (6 if c == 0 else 2)
            out += l29(v + j * q)
    assert any(out[2 * g.uw:3 * g.uw]), "a finite point with ZZ == 0 limbs"
    return out


def dec_point(g, words, zz_pow):
    """register-form words -> (affine point or None, the four coordinates' values).  Asserts the invariant: N-form, X < 6p, others < 2p,
    ZZ^3 == ZZZ^2."""
    q, F = M.Q, g.F
    vals = [[v29(words[c * g.uw + 9 * i:c * g.uw + 9 * i + 9]) for i in range(g.n)] for c in range(4)]
    if not any(words[2 * g.uw:3 * g.uw]):
        return None, vals
    for c in range(4):
        for i in range(g.n):
            l = [int(x) for x in words[c * g.uw + 9 * i:c * g.uw + 9 * i + 9]]
            assert is_n(l), "coordinate %d not N-form: %s" % (c, hexw(l))
            assert vals[c][i] < (6 if c == 0 else 2) * q, "coordinate %d = %x breaks the invariant (< %dp)" % (c, vals[c][i], 6 if c == 0 else 2)
    ri, zi = pow(RU, -1, q), pow(1 << zz_pow, -1, q)
    X, Y = (g.scale(g.el(vals[c]), ri) for c in (0, 1))
    ZZ, ZZZ = (g.scale(g.el(vals[c]), zi) for c in (2, 3))
    assert F.mul(F.mul(ZZ, ZZ), ZZ) == F.mul(ZZZ, ZZZ), "ZZ^3 != ZZZ^2"
    assert ZZ != F.zero, "ZZ == 0 mod p with non-zero limbs"
    return (F.mul(X, F.inv(ZZ)), F.mul(Y, F.inv(ZZZ))), vals


def _lift_sets(g, rnd):
    zero = [[0] * g.n for _ in range(4)]
    top = [[5] * g.n] + [[1] * g.n for _ in range(3)]
    mixed = [[rnd.randrange(6) for _ in range(g.n)]] + [[rnd.randrange(2) for _ in range(g.n)] for _ in range(3)]
    return [("", zero), ("+max_lift", top), ("+lift", mixed)]


def _rand_z(g, rnd):
    while True:
        z = g.el([rnd.randrange(M.Q) for _ in range(g.n)])
        if z != g.F.zero:
            return z


def _one(g):
    return g.el([1] + [0] * (g.n - 1))


class GroupOp(Op):
    """what: DOUBLE_AFFINE, DOUBLE, ADD_MIXED, RADD, RECORD_TRIP, RADD_QUAD, PAIR_ADD_MIXED (csrc/selftest_dev_ops.hpp: group_op)."""

    def __init__(self, g, what):
        uw, fw = g.uw, g.fw
        A, R = 4 * uw, 4 * fw
        shape = {"DOUBLE_AFFINE": (2 * fw, A, 1), "DOUBLE": (A, A, 1), "ADD_MIXED": (A + 2 * fw + 1, A + R, 1), "RADD": (2 * A, A + R, 1),
                 "RECORD_TRIP": (A, R + A + R, 1), "RADD_QUAD": (2 * A, A + R, 4), "PAIR_ADD_MIXED": (A + 2 * fw + 1, 2 * uw + 2 * fw, 2)}[what]
        super().__init__("%s_%s" % (g.name, what), shape[0], shape[1], fields=(0,), group=shape[2], chain=(g.n == 1))
        self.g, self.what = g, what
        self.base = {"RADD_QUAD": "RADD", "PAIR_ADD_MIXED": "ADD_MIXED"}.get(what)    # the one-lane op with the same cases

    # -- cases: built once per (group, base op) so the lane-group forms get the very same operands
    def cases(self, which):
        g, what = self.g, self.base or self.what
        n_random = N_RANDOM_GROUPS if self.group > 1 else N_RANDOM
        rnd = _rng("%s_%s" % (g.name, what), 0)
        named, more = pool(g)
        rows = []
        if what == "DOUBLE_AFFINE":
            pts = named + [("random", rnd.choice(more)) for _ in range(n_random)]
            return [(n, g.coord_words(pt[0]) + g.coord_words(pt[1])) for n, pt in pts]
        if what in ("DOUBLE", "RECORD_TRIP"):
            zp = 261 if what == "DOUBLE" else 266
            rows.append(("infinity", enc_point(g, None, None, None, zp)))
            for n, pt in named:
                for ln, lifts in _lift_sets(g, rnd):
                    rows.append((n + ",z=1" + ln, enc_point(g, pt, _one(g), lifts, zp)))
                    rows.append((n + ln, enc_point(g, pt, _rand_z(g, rnd), lifts, zp)))
            for _ in range(n_random):
                rows.append(("random", enc_point(g, rnd.choice(more), _rand_z(g, rnd), _lift_sets(g, rnd)[2][1], zp)))
            return rows
        mixed = what == "ADD_MIXED"
        zp = 266 if mixed else 261

        def second(pt, neg, z, lifts):
            if mixed:      # a canonical affine base and the sign bit: never infinity (the kernels skip the zero record)
                return g.coord_words(pt[0]) + g.coord_words(pt[1]) + [int(neg)]
            return enc_point(g, g.neg(pt) if neg and pt is not None else pt, z, lifts, 261)

        lsets = _lift_sets(g, rnd)
        zero = lsets[0][1]
        special = []
        for n, pt in named:
            special.append(("acc=inf , o=" + n, None, pt, False))
            special.append(("acc=inf , o=-" + n, None, pt, True))
            special.append(("o=acc (double) " + n, pt, pt, False))
            special.append(("o=-acc (x equal, y opposite: infinity) " + n, pt, pt, True))
        for (na, a), (nb, b) in ((named[0], named[1]), (named[1], named[0]), (named[0], named[2]), (named[3], named[1]), (named[4], named[0]),
                                 (named[-1], named[0]), (named[-1], named[4])):
            special.append(("%s + %s" % (na, nb), a, b, False))
            special.append(("%s - %s" % (na, nb), a, b, True))
        i = 0
        for n, a, b, neg in special:
            for ln, lifts in lsets:                                    # the accumulator as itself and as lazy twins
                for zn, z in (("", _rand_z(g, rnd)), (",acc z=1", _one(g))):
                    i += 1
                    rows.append((n + ln + zn, enc_point(g, a, z, lifts, zp) + second(b, neg, _rand_z(g, rnd), lsets[i % 3][1])))
                    # an ordinary case next to every special one: neighbouring lanes / groups hold different data
                    rows.append(("ordinary", enc_point(g, rnd.choice(more), _rand_z(g, rnd), lsets[2][1], zp) + second(rnd.choice(named[:5])[1], i & 1, _rand_z(g, rnd), zero)))
        if not mixed:
            for n, pt in named:
                rows.append(("o=inf , acc=" + n, enc_point(g, pt, _rand_z(g, rnd), lsets[1][1], zp) + enc_point(g, None, None, None, 261)))
            rows.append(("acc=inf , o=inf", enc_point(g, None, None, None, zp) * 2))
        for _ in range(n_random):
            a, b = rnd.choice(more), rnd.choice(more)
            rows.append(("random", enc_point(g, a, _rand_z(g, rnd), _lift_sets(g, rnd)[2][1], zp) + second(b, rnd.random() < 0.5, _rand_z(g, rnd), _lift_sets(g, rnd)[2][1])))
        return rows

    # -- reference: the affine result by bn254_model
    def expect(self, which, inw):
        g, what = self.g, self.base or self.what
        A, fw, q = 4 * g.uw, g.fw, M.Q
        ri = _rinv(q)

        def affine(words):
            cs = [v32(words[8 * i:8 * i + 8]) for i in range(2 * g.n)]
            assert all(c < q for c in cs)
            pt = (g.el([c * ri % q for c in cs[:g.n]]), g.el([c * ri % q for c in cs[g.n:]]))
            assert g.on_curve(pt)
            return pt
        if what == "DOUBLE_AFFINE":
            pt = affine(inw)
            return {"pt": g.add(pt, pt)}
        if what == "DOUBLE":
            pt, _ = dec_point(g, inw, 261)
            return {"pt": g.add(pt, pt)}
        if what == "RECORD_TRIP":
            pt, vals = dec_point(g, inw, 266)
            return {"pt": pt, "vals": vals}
        acc, _ = dec_point(g, inw[:A], 266 if what == "ADD_MIXED" else 261)
        assert g.on_curve(acc)
        if what == "ADD_MIXED":
            o = affine(inw[A:A + 2 * fw])
            assert inw[A + 2 * fw] in (0, 1)
            o = g.neg(o) if inw[A + 2 * fw] else o
        else:
            o, _ = dec_point(g, inw[A:], 261)
        return {"pt": g.add(acc, o)}

    def _rec_check(self, vals, rec_words, scale_zz):
        """a record holds the canonical values of the four coordinates in the 2^261 domain"""
        g, q = self.g, M.Q
        want = []
        for c in range(4):
            s = scale_zz if c >= 2 else 1
            want += sum((w32(v * s % q) for v in vals[c]), [])
        assert [int(x) for x in rec_words] == want, "record %s, want %s" % (hexw(rec_words), hexw(want))

    def verify(self, which, inw, outw, exp):
        g, what, q = self.g, self.what, M.Q
        A, R = 4 * g.uw, 4 * g.fw
        outw = [int(x) for x in outw]
        down5 = pow(32, -1, q)        # 2^266 -> 2^261
        if what == "RECORD_TRIP":
            rec, back, rec2 = outw[:R], outw[R:R + A], outw[R + A:]
            if exp["pt"] is None:
                assert not any(outw), "infinity must give the zero record and zero limbs"
                return
            self._rec_check(exp["vals"], rec, down5)
            pt, vals = dec_point(g, back, 266)
            assert pt == exp["pt"] and all(v < q for v in vals[0] + vals[1]), "xyzzu_from_r(xyzzu_to_r(a)) is another point"
            assert rec2 == rec, "xyzzr_store(xyzzr_load(rec)) != rec"
            return
        if what == "PAIR_ADD_MIXED":
            raise AssertionError("verify the pair form with verify_pair (both lanes)")
        acc_form = what in ("DOUBLE_AFFINE", "ADD_MIXED")
        pt, vals = dec_point(g, outw[:A], 266 if acc_form else 261)
        assert pt == exp["pt"], "got %s, want %s" % (pt, exp["pt"])
        if what in ("ADD_MIXED", "RADD", "RADD_QUAD"):
            if pt is None:
                assert not any(outw[A:]), "infinity must give the zero record"
            else:
                self._rec_check(vals, outw[A:], down5 if acc_form else 1)

    def verify_pair(self, inw, even, odd, exp):
        """the pair form: the even lane returns (X, ZZ) and the record's x, zz; the odd lane (Y, ZZZ) and y, zzz"""
        g = self.g
        uw, fw = g.uw, g.fw
        even, odd = [int(x) for x in even], [int(x) for x in odd]
        acc = even[:uw] + odd[:uw] + even[uw:2 * uw] + odd[uw:2 * uw]
        rec = even[2 * uw:2 * uw + fw] + odd[2 * uw:2 * uw + fw] + even[2 * uw + fw:] + odd[2 * uw + fw:]
        if exp["pt"] is None:
            assert not any(even[uw:2 * uw]) and not any(odd[uw:2 * uw]), "infinity: z must be literal zeros in BOTH lanes"
            assert not any(rec), "infinity must give the zero record"
            return rec
        pt, vals = dec_point(g, acc, 266)
        assert pt == exp["pt"], "got %s, want %s" % (pt, exp["pt"])
        self._rec_check(vals, rec, pow(32, -1, M.Q))
        return rec


# ---- Jacobian forms (scalar_mul.hip, point_fft_g2.hip): X, Y, Z in U-form, every coordinate in the 2^261 domain
JAC_BOUNDS = {1: (6, 2, 2), 2: (7, 3, 3)}     # curveu.hpp: G1  X < 6p, Y < 2p, Z < 2p;   G2 per component  X < 7p, Y <= 3p, Z < 3p


def enc_jac(g, pt, z, lifts):
    """X = x z^2, Y = y z^3, Z = z (times 2^261), component i of coordinate c lifted by lifts[c][i] * p inside JAC_BOUNDS; None: zeros"""
    if pt is None:
        return [0] * (3 * g.uw)
    F, q = g.F, M.Q
    zz = F.mul(z, z)
    coords = [F.mul(pt[0], zz), F.mul(pt[1], F.mul(zz, z)), z]
    out = []
    for c, e in enumerate(coords):
        for i, v in enumerate(g.comps(g.scale(e, RU % q))):
            assert 0 <= lifts[c][i] < JAC_BOUNDS[g.n][c]
            out += l29(v + lifts[c][i] * q)
    assert any(out[2 * g.uw:]), "a finite point with Z == 0 limbs"
    return out


def dec_jac(g, words):
    """-> (affine point or None, coordinate values); asserts N-form and JAC_BOUNDS"""
    q, F = M.Q, g.F
    vals = [[v29(words[c * g.uw + 9 * i:c * g.uw + 9 * i + 9]) for i in range(g.n)] for c in range(3)]
    if not any(words[2 * g.uw:3 * g.uw]):
        return None, vals
    for c in range(3):
        for i in range(g.n):
            l = [int(x) for x in words[c * g.uw + 9 * i:c * g.uw + 9 * i + 9]]
            assert is_n(l), "coordinate %d not N-form: %s" % (c, hexw(l))
            k = JAC_BOUNDS[g.n][c]
            assert vals[c][i] < k * q or (g.n == 2 and c == 1 and vals[c][i] == k * q), "coordinate %d = %x breaks the invariant (%dp)" % (c, vals[c][i], k)
    ri = pow(RU, -1, q)
    X, Y, Z = (g.scale(g.el(vals[c]), ri) for c in range(3))
    assert Z != F.zero, "Z == 0 mod p with non-zero limbs"
    zi = F.inv(Z)
    zi2 = F.mul(zi, zi)
    return (F.mul(X, zi2), F.mul(Y, F.mul(zi2, zi))), vals


def _jac_lifts(g, rnd):
    b = JAC_BOUNDS[g.n]
    return [("", [[0] * g.n for _ in range(3)]), ("+max_lift", [[b[c] - 1] * g.n for c in range(3)]),
            ("+lift", [[rnd.randrange(b[c]) for _ in range(g.n)] for c in range(3)])]


class JacOp(Op):
    """what: DOUBLE (jacu_double / jacu2_double), ADD_MIXED (jacu_add_mixed, G1), ADD_TAB (tab_entry of q, then add_tab), TAB_PSI (G2:
    tab_entry of q, then jacu2_tab_psi with constants cx, cy in U-form, components < 2p)."""

    def __init__(self, g, what):
        uw = g.uw
        shape = {"DOUBLE": (3 * uw, 3 * uw), "ADD_MIXED": (5 * uw + 1, 3 * uw), "ADD_TAB": (6 * uw + 1, 5 * uw), "TAB_PSI": (5 * uw, 5 * uw)}[what]
        super().__init__("%s_JAC_%s" % (g.name, what), shape[0], shape[1], fields=(0,))
        self.g, self.what = g, what

    def cases(self, which):
        g, what, q = self.g, self.what, M.Q
        rnd = _rng(self.name, 0)
        named, more = pool(g)
        rows = []
        if what in ("DOUBLE", "TAB_PSI"):
            def tail():
                if what == "DOUBLE":
                    return []
                return sum((l29(rnd.randrange(q) + rnd.randrange(2) * q) for _ in range(4)), [])      # cx, cy: components < 2p, N-form
            if what == "DOUBLE":
                rows.append(("infinity", enc_jac(g, None, None, None)))
            for n, pt in named:
                for ln, lifts in _jac_lifts(g, rnd):
                    rows.append((n + ",z=1" + ln, enc_jac(g, pt, _one(g), lifts) + tail()))
                    rows.append((n + ln, enc_jac(g, pt, _rand_z(g, rnd), lifts) + tail()))
            if what == "TAB_PSI":
                top = l29(2 * q - 1)
                rows.append(("cx, cy = 2p-1 , max lift", enc_jac(g, named[4][1], _rand_z(g, rnd), _jac_lifts(g, rnd)[1][1]) + top * 4))
                rows.append(("cx, cy = 0", enc_jac(g, named[4][1], _rand_z(g, rnd), _jac_lifts(g, rnd)[1][1]) + [0] * 36))
            for _ in range(N_RANDOM):
                rows.append(("random", enc_jac(g, rnd.choice(more), _rand_z(g, rnd), _jac_lifts(g, rnd)[2][1]) + tail()))
            return rows
        mixed = what == "ADD_MIXED"

        def second(pt, neg, z, lifts):
            if mixed:      # x2, y2 in the 2^261 domain, N-form, < 2p: z = 1 with the x, y lifts capped at one p
                w = enc_jac(g, pt, _one(g), [[min(1, j) for j in lifts[0]], [min(1, j) for j in lifts[1]], [0] * g.n])
                return w[:2 * g.uw] + [int(neg)]
            return enc_jac(g, pt, z, lifts) + [int(neg)]

        lsets = _jac_lifts(g, rnd)
        special = []
        for n, pt in named:
            special += [("acc=inf , o=" + n, None, pt, False), ("acc=inf , o=-" + n, None, pt, True), ("o=acc (double) " + n, pt, pt, False),
                        ("o=-acc (x equal, y opposite: infinity) " + n, pt, pt, True)]
        for (na, a), (nb, b) in ((named[0], named[1]), (named[1], named[0]), (named[0], named[2]), (named[3], named[1]), (named[4], named[0]),
                                 (named[-1], named[4])):
            special += [("%s + %s" % (na, nb), a, b, False), ("%s - %s" % (na, nb), a, b, True)]
        i = 0
        for n, a, b, neg in special:
            for ln, lifts in lsets:
                for zn, z in (("", _rand_z(g, rnd)), (",acc z=1", _one(g))):
                    i += 1
                    rows.append((n + ln + zn, enc_jac(g, a, z, lifts) + second(b, neg, _rand_z(g, rnd), lsets[i % 3][1])))
                    rows.append(("ordinary", enc_jac(g, rnd.choice(more), _rand_z(g, rnd), lsets[2][1]) + second(rnd.choice(named[:5])[1], i & 1, _rand_z(g, rnd), lsets[0][1])))
        for _ in range(N_RANDOM):
            rows.append(("random", enc_jac(g, rnd.choice(more), _rand_z(g, rnd), _jac_lifts(g, rnd)[2][1]) +
                         second(rnd.choice(more), rnd.random() < 0.5, _rand_z(g, rnd), _jac_lifts(g, rnd)[2][1])))
        return rows

    def expect(self, which, inw):
        g, what, q = self.g, self.what, M.Q
        J, uw = 3 * g.uw, g.uw
        acc, vals = dec_jac(g, inw[:J])
        assert g.on_curve(acc)
        if what == "DOUBLE":
            return {"pt": g.add(acc, acc)}
        if what == "TAB_PSI":
            assert acc is not None
            cs = [[int(x) for x in inw[J + 9 * i:J + 9 * i + 9]] for i in range(4)]
            assert all(is_n(c) and v29(c) < 2 * q for c in cs)
            return {"vals": vals, "cx": (v29(cs[0]), v29(cs[1])), "cy": (v29(cs[2]), v29(cs[3]))}
        if what == "ADD_MIXED":
            x2, y2 = inw[J:J + uw], inw[J + uw:J + 2 * uw]
            assert is_n([int(v) for v in x2]) and is_n([int(v) for v in y2]) and v29(x2) < 2 * q and v29(y2) < 2 * q
            ri = pow(RU, -1, q)
            o = (v29(x2) * ri % q, v29(y2) * ri % q)
            neg = inw[J + 2 * uw]
        else:
            o, ovals = dec_jac(g, inw[J:2 * J])
            assert o is not None                     # "t != infinity"
            neg = inw[2 * J]
        assert g.on_curve(o) and neg in (0, 1)
        exp = {"pt": g.add(acc, g.neg(o) if neg else o)}
        if what == "ADD_TAB":
            exp["z"] = g.el(ovals[2])
        return exp

    def verify(self, which, inw, outw, exp):
        g, what, q, F = self.g, self.what, M.Q, self.g.F
        J, uw = 3 * g.uw, g.uw
        outw = [int(x) for x in outw]
        ri = pow(RU, -1, q)

        def coord(words, bound, inclusive=False):
            out = []
            for i in range(g.n):
                l = words[9 * i:9 * i + 9]
                assert is_n(l), "not N-form: %s" % hexw(l)
                assert v29(l) < bound or (inclusive and v29(l) == bound), "value %x is not below the stated bound %x" % (v29(l), bound)
                out.append(v29(l) % q)
            return g.el(out)
        if what == "TAB_PSI":
            conj = lambda e: (e[0], -e[1] % q)                                   # noqa: E731
            X, Y, Z = (g.el([v % q for v in exp["vals"][c]]) for c in range(3))
            cx, cy = ((c[0] % q, c[1] % q) for c in (exp["cx"], exp["cy"]))
            zz = g.scale(F.mul(Z, Z), ri)
            zzz = g.scale(F.mul(Z, zz), ri)
            want = [g.scale(F.mul(conj(X), cx), ri), g.scale(F.mul(conj(Y), cy), ri), conj(Z), conj(zz), conj(zzz)]
            bounds = [(12 * q // 10, False), (11 * q // 10, False), (3 * q, True), (2 * q, True), (2 * q, True)]     # "X < 1.2p, Y < 1.1p, Z_1 <= 3p, ZZ_1, ZZZ_1 <= 2p"
            for c in range(5):
                got = coord(outw[c * uw:(c + 1) * uw], *bounds[c])
                assert got == want[c], "coordinate %d: got %s, want %s" % (c, got, want[c])
            return
        pt, _ = dec_jac(g, outw[:J])
        assert pt == exp["pt"], "got %s, want %s" % (pt, exp["pt"])
        if what == "ADD_TAB":
            Z = g.el([v % q for v in g.comps(exp["z"])])
            zz = g.scale(F.mul(Z, Z), ri)
            assert coord(outw[J:J + uw], 2 * q) == zz and coord(outw[J + uw:], 2 * q) == g.scale(F.mul(Z, zz), ri), "the entry's ZZ / ZZZ"


JAC_OPS = [JacOp(G1, "DOUBLE"), JacOp(G1, "ADD_MIXED"), JacOp(G1, "ADD_TAB"), JacOp(G2, "DOUBLE"), JacOp(G2, "ADD_TAB"), JacOp(G2, "TAB_PSI")]

GROUP_WHATS = ["DOUBLE_AFFINE", "DOUBLE", "ADD_MIXED", "RADD", "RECORD_TRIP", "RADD_QUAD", "PAIR_ADD_MIXED"]
GROUP_OPS = [GroupOp(g, w) for g in (G1, G2) for w in GROUP_WHATS]

ALL_OPS = FP_OPS + FQ2_OPS + U_OPS + F2U_OPS + GROUP_OPS + JAC_OPS
BY_NAME = {op.name: op for op in ALL_OPS}
CODES = {op.name: i for i, op in enumerate(ALL_OPS)}      # the enum's order (a test compares it with include/mi355zk.h)


# ---- chains: 64 mixed additions into one accumulator, each step's result fed back as the next step's operand
CHAIN_STEPS, N_CHAINS = 64, 32
CHAIN_PLANTS = {0: "onto infinity", 1: "repeat of step 0 (doubling)", 20: "negation of the running sum (infinity)", 21: "onto infinity again",
                40: "the running sum itself (doubling of a lazily reduced accumulator)"}


def chain_schedule(g, chain):
    """-> [(affine base, negate, running sum after the step)]: random signed bases with CHAIN_PLANTS at their fixed positions"""
    rnd = _rng("chain" + g.name, chain)
    named, more = pool(g)
    pts = more + [pt for _, pt in named]
    acc, out = None, []
    for step in range(CHAIN_STEPS):
        pt, neg = rnd.choice(pts), rnd.random() < 0.5
        if step == 1:
            pt, neg = out[0][0], out[0][1]
        elif step == 20:
            pt, neg = acc, True
        elif step == 40:
            pt, neg = acc, False
        assert pt is not None                    # a base is never infinity
        acc = g.add(acc, g.neg(pt) if neg else pt)
        out.append((pt, neg, acc))
    assert out[1][2] == g.add(out[0][2], out[0][2]) and out[20][2] is None and out[21][2] is not None
    return out


def class_counts(op, which):
    out: dict = {}
    for cls, _ in op.table(which):
        key = cls if cls in ("random", "ordinary") or cls.startswith("random") else "named"
        out[key] = out.get(key, 0) + 1
    return out
