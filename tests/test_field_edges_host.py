"""The edge-operand table of tests/field_edge_vectors.py, without a GPU: every case lies inside the contract of its primitive and has a
big-int reference (Op.expect asserts both), the host-compiled hooks (mi355zk_selftest_u_*) return what the reference says for the ops that
have one, the Python column model of the device's Fp product covers what it claims, and the op set is the header's enum.  The GPU leg
(tests/test_gpu_field_edges.py) runs the same table through the device."""
import os
import re

import numpy as np
import pytest

import field_edge_vectors as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = [(op.name, which) for op in V.ALL_OPS for which in op.fields]


@pytest.fixture(scope="module")
def lib():
    import phase2_bn254_amd as zk

    return zk.lib.load()


def header_enum():
    text = open(os.path.join(ROOT, "include", "mi355zk.h")).read()
    body = re.search(r"enum mi355zk_devop \{(.*?)\};", text, flags=re.S).group(1)
    names = re.findall(r"MI355ZK_DEVOP_(\w+)", body)
    assert names[-1] == "COUNT"
    return names[:-1]


def test_the_table_and_the_enum_have_the_same_ops():
    """a primitive cannot be added to the device hook without vectors, nor vectors without the hook; the codes are the enum's order"""
    names = header_enum()
    assert names == [op.name for op in V.ALL_OPS]
    assert [V.CODES[n] for n in names] == list(range(len(names)))
    text = open(os.path.join(ROOT, "include", "mi355zk.h")).read()
    assert int(re.search(r"#define MI355ZK_DEVOP_CHAIN (\w+)", text).group(1), 16) == V.CHAIN
    # the kernels instantiate these u_sub<K, S>, f2u_mul / sqr / sub<K>: the list comes from the sources, not from memory
    src = ""
    csrc = os.path.join(ROOT, "phase2-bn254_amd", "csrc")
    for f in sorted(os.listdir(csrc)):
        if not f.startswith("selftest_dev") and f != "field_ops.hip":     # (field_ops.hip: the HOST replay of the pair additions)
            src += open(os.path.join(csrc, f)).read()
    ks = {(int(a), int(b)) for a, b in re.findall(r"\bu_sub<(\d+), ?(\d+)>", src)}
    ks |= {(int(k), 1) for k in re.findall(r"\bf2u_sub<(\d+)>", src)} | {(int(k), 1) for k in re.findall(r"\bf2u_(?:mul|sqr)<(\d+)>", src)}
    ks.discard((6, 1))   # f2u_sqr<6> -> u_sub<6, 1> appears only inside it: covered by F2U_SQR_6
    assert ks == set(V.U_SUB_KS), sorted(ks)
    for what in ("mul", "sqr", "sub"):
        want = sorted({int(k) for k in re.findall(r"\bf2u_%s<(\d+)>" % what, src)})
        assert want == sorted(op.K for op in V.F2U_OPS if op.what == what.upper()), (what, want)


@pytest.mark.parametrize("name,which", ALL)
def test_every_case_is_inside_its_contract_and_has_a_reference(name, which):
    op = V.BY_NAME[name]
    rows = op.table(which)
    assert len(rows) >= (V.N_RANDOM_GROUPS if op.group > 1 else V.N_RANDOM)
    assert sum(1 for cls, _ in rows if cls.startswith("random")) == (V.N_RANDOM_GROUPS if op.group > 1 else V.N_RANDOM)
    for cls, inw in rows:
        try:
            op.expect(which, inw)
        except AssertionError as e:
            raise AssertionError("%s: %s" % (op.describe(which, cls, inw), e)) from None


def _host_call(lib, op, which, inw):
    """the host-compiled hook for this op, or None"""
    u32 = lambda l: np.array(l, dtype=np.uint32)   # noqa: E731
    h = op.host
    if h == "u_mul":
        a, b, out = u32(inw[:9]), u32(inw[9:]), np.zeros(9, np.uint32)
        assert lib.mi355zk_selftest_u_mul(which, a.ctypes.data, b.ctypes.data, out.ctypes.data) == 0
        return list(out)
    if h == "u_mul_shoup":
        a, w, out, wq = u32(inw[:9]), u32(inw[9:]), np.zeros(9, np.uint32), np.zeros(9, np.uint32)
        assert lib.mi355zk_selftest_u_mul_shoup(which, a.ctypes.data, w.ctypes.data, out.ctypes.data, wq.ctypes.data) == 0
        return list(out) + list(wq)
    if isinstance(h, tuple):
        a, b, out = u32(inw[:9]), u32(inw[9:]), np.zeros(9, np.uint32)
        assert lib.mi355zk_selftest_u_sub(which, h[1][0], h[1][1], a.ctypes.data, b.ctypes.data, out.ctypes.data) == 0
        return list(out)
    if h == "u_pack_in":
        a, out = u32(inw), np.zeros(9, np.uint32)
        assert lib.mi355zk_selftest_u_pack(which, a.ctypes.data, out.ctypes.data, None, None) == 0
        return list(out)
    if h == "u_pack_out":
        a, out = u32(inw), np.zeros(8, np.uint32)
        assert lib.mi355zk_selftest_u_pack(which, None, None, a.ctypes.data, out.ctypes.data) == 0
        return list(out)
    if h == "u_reduce32":
        a, out = u32(inw), np.zeros(8, np.uint32)
        assert lib.mi355zk_selftest_u_reduce32(which, a.ctypes.data, out.ctypes.data) == 0
        return list(out)
    return None


@pytest.mark.parametrize("name,which", [(n, w) for n, w in ALL if V.BY_NAME[n].host])
def test_host_hooks_agree_with_the_reference(lib, name, which):
    op = V.BY_NAME[name]
    for cls, inw in op.table(which):
        out = _host_call(lib, op, which, inw)
        try:
            op.verify(which, inw, out, op.expect(which, inw))
        except AssertionError as e:
            raise AssertionError("%s: %s" % (op.describe(which, cls, inw), e)) from None


@pytest.mark.parametrize("gname", ["G1", "G2"])
def test_chains_through_the_host_accumulators(lib, gname):
    """the chains of field_edge_vectors.chain_schedule (64 signed additions with an infinity, a repeat and a negation planted) through the host-
    compiled bucket accumulators -- mi355zk_selftest_g1_accumulate / _g2_accumulate: the U-form addition (mode 1), the accumulator through a
    record after every third point (2), the replay of the pair-per-bucket addition (3) -- at EVERY prefix length against bn254_model"""
    import bn254_model as M

    g = V.G1 if gname == "G1" else V.G2
    fn = lib.mi355zk_selftest_g1_accumulate if g.n == 1 else lib.mi355zk_selftest_g2_accumulate
    q, ri = M.Q, pow(1 << 256, -1, M.Q)
    for chain in range(4):
        sched = V.chain_schedule(g, chain)
        pts = np.array([g.coord_words(pt[0]) + g.coord_words(pt[1]) for pt, _, _ in sched], dtype=np.uint32)
        neg = np.array([int(n) for _, n, _ in sched], dtype=np.uint8)
        for mode in (1, 2, 3):
            for n in range(1, V.CHAIN_STEPS + 1):
                out = np.zeros(32 * g.n, np.uint32)
                assert fn(mode, pts.ctypes.data, neg.ctypes.data, n, out.ctypes.data) == 0
                c = [g.el([V.v32(out[8 * (g.n * k + i):8 * (g.n * k + i) + 8]) * ri % q for i in range(g.n)]) for k in range(4)]
                got = None if c[2] == g.F.zero else (g.F.mul(c[0], g.F.inv(c[2])), g.F.mul(c[1], g.F.inv(c[3])))
                assert got == sched[n - 1][2], "%s chain %d mode %d after step %d (%s)" % (gname, chain, mode, n - 1, V.CHAIN_PLANTS.get(n - 1, "random base"))


def test_the_schedule_model_is_the_generated_file():
    """fp_mul_schedule() restates tools/gen_mont_mul.py: as many multiply-accumulates, and as many carry absorbers, as the .inc holds"""
    inc = open(os.path.join(ROOT, "phase2-bn254_amd", "csrc", "mont_mul_gfx950.inc")).read()
    assert inc.count("v_mad_u64_u32") == inc.count("v_addc_co_u32") == len(V.FP_MUL_MACS) == 128
    for k, seq in enumerate(V.FP_MUL_SCHEDULE):
        block = inc.split("// column %d\n" % k)[1].split("// column")[0]
        assert block.count("v_mad_u64_u32") == len(seq), k


# what the NAMED cases of FP_MUL reach in the column model: the values of every m[k], of every column's third word, the absorbers that fired
def _coverage(which):
    p = V.MODS[which]
    op = V.BY_NAME["FP_MUL"]
    named = [(cls, inw) for cls, inw in op.table(which) if cls != "random"]
    m_seen = [set() for _ in range(8)]
    third_seen = [set() for _ in range(16)]
    carried, sides = set(), set()
    for cls, inw in named:
        a, b = V.v32(inw[:8]), V.v32(inw[8:])
        r, m, third, car = V.fp_mul_columns(a, b, p)
        assert r % p == a * b * pow(1 << 256, -1, p) % p and r < 2 * p, cls          # the model is a Montgomery product
        for k in range(8):
            m_seen[k].add(m[k])
        for k in range(16):
            third_seen[k].add(third[k])
        carried |= car
        sides.add(r >= p)
    return m_seen, third_seen, carried, sides


@pytest.mark.parametrize("which", [0, 1])
def test_column_model_coverage_of_the_fp_product(which):
    """over the NAMED cases of FP_MUL: every m[k] takes 0 and ffffffff, the third word of every column takes 0 and the largest count the
    column can reach, every carry absorber that can fire does, and the value before reduce_once falls on both sides of p"""
    p = V.MODS[which]
    m_seen, third_seen, carried, sides = _coverage(which)
    for k in range(8):
        assert 0 in m_seen[k] and 0xFFFFFFFF in m_seen[k], k
    assert sides == {True, False}
    # an upper bound of a column's third word: (sum of the largest terms + the largest carry-in) >> 64, limbs at ffffffff / p's own
    P = V.w32(p)
    top_a = p >> 224
    carry_in = 0
    cannot = set()      # absorbers that cannot fire: even with every term at its largest the running sum stays below 2^64
    for k, seq in enumerate(V.FP_MUL_SCHEDULE):
        total = carry_in
        for n, (kind, i, j) in enumerate(seq):
            x = (top_a if i == 7 else V.MASK32) if kind == "ab" else V.MASK32
            y = (top_a if j == 7 else V.MASK32) if kind == "ab" else P[j]
            total += x * y
            if total < 1 << 64:
                cannot.add((k, n))
        ub = total >> 64
        carry_in = total >> 32
        assert 0 in third_seen[k], k
        # `ub` is an upper bound, not the maximum: it puts every limb of a, b and m at ffffffff at once (a, b < p and m = -a b / p do not allow
        # that) and feeds each column the previous column's own bound as carry-in, so its excess compounds towards the middle columns.  The true
        # maximum is not known in closed form; the directed operands reach ub itself in the outer columns and ub - 1 or ub - 2 in columns 5 - 7.
        # The assertion therefore fixes how far below the bound the table may stay (2); what makes a lost carry visible is not this figure but
        # the absorber-by-absorber test below.
        if seq:
            assert max(third_seen[k]) >= max(0, ub - 2), (k, max(third_seen[k]), ub)
    never = {mac for mac in V.FP_MUL_MACS if mac not in carried}
    # out of reach: those, and the first accumulation of a column (it would need the carry-in word and both limbs at their maxima at once)
    assert never <= cannot | {(k, 0) for k in range(16)}, sorted(never - cannot)


@pytest.mark.parametrize("which", [0, 1])
def test_a_missing_carry_absorber_is_caught_by_named_cases(which):
    """the mutation of a careless edit -- one v_addc_co_u32 deleted from a middle column of mont_mul_gfx950.inc -- on the model: for EVERY
    absorber that can fire, a named case gives a wrong product; the random cases alone would not be relied on"""
    p = V.MODS[which]
    op = V.BY_NAME["FP_MUL"]
    named = [(cls, V.v32(inw[:8]), V.v32(inw[8:])) for cls, inw in op.table(which) if cls != "random"]
    _, _, carried, _ = _coverage(which)
    for mac in sorted(carried):
        hit = None
        for cls, a, b in named:
            if mac in V.fp_mul_columns(a, b, p)[3]:
                assert V.fp_mul_columns(a, b, p, drop=mac)[0] % p != a * b * pow(1 << 256, -1, p) % p
                hit = cls
                break
        assert hit is not None, mac


def test_dev_op_rejects_bad_arguments_without_a_device(lib):
    import phase2_bn254_amd as zk

    a, out = np.zeros(16, np.uint32), np.zeros(8, np.uint32)
    f = lib.mi355zk_selftest_dev_op
    bad = zk.lib.ERR_BAD_ARGS
    assert f(len(V.ALL_OPS), 0, a.ctypes.data, 16, out.ctypes.data, 8, 1) == bad          # unknown op
    assert f(-1, 0, a.ctypes.data, 16, out.ctypes.data, 8, 1) == bad
    assert f(V.CODES["FP_MUL"], 0, a.ctypes.data, 15, out.ctypes.data, 8, 1) == bad       # word counts
    assert f(V.CODES["FP_MUL"], 0, a.ctypes.data, 16, out.ctypes.data, 9, 1) == bad
    assert f(V.CODES["FP_MUL"], 2, a.ctypes.data, 16, out.ctypes.data, 8, 1) == bad       # which
    assert f(V.CODES["FP_MUL"], 0, None, 16, out.ctypes.data, 8, 1) == bad
    assert f(V.CODES["FP_MUL"], 0, a.ctypes.data, 16, out.ctypes.data, 8, 0) == bad
    assert f(V.CODES["FP_MUL"] | V.CHAIN, 0, a.ctypes.data, 16, out.ctypes.data, 8, 1) == bad   # no ZK_CHAIN_MAD build of an Fp op
    assert f(V.CODES["FQ2_NEG"], 1, a.ctypes.data, 16, out.ctypes.data, 16, 1) == bad     # Fq2 over Fr
    q = V.BY_NAME["G1_RADD_QUAD"]
    big_in, big_out = np.zeros(q.in_words * 4, np.uint32), np.zeros(q.out_words * 4, np.uint32)
    assert f(V.CODES[q.name], 0, big_in.ctypes.data, q.in_words, big_out.ctypes.data, q.out_words, 3) == bad   # not whole quads
    for op in V.ALL_OPS:   # the shapes of the table are the shapes of the hook: a wrong count is refused, so a right one is what passes on the GPU
        assert f(V.CODES[op.name], 0, a.ctypes.data, op.in_words + 1, out.ctypes.data, op.out_words, op.group) == bad, op.name
        assert f(V.CODES[op.name], 0, a.ctypes.data, op.in_words, out.ctypes.data, op.out_words + 1, op.group) == bad, op.name
