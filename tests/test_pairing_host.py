"""The pairing arithmetic of phase2-bn254_amd/csrc/pairing.hpp, compiled for the host, against the independent big-int model
(tests/pairing_model.py) -- no GPU needed: the model's own sanity, every tower primitive through mi355zk_selftest_pairing_op, the host
product mi355zk_bn254_pairing_product against tests/golden/pairing_golden.json byte for byte, and the argument checks of the Python layer."""
import ctypes as C
import json
import os
import random

import numpy as np
import pytest

import bn254_model as M
import pairing_model as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q, R = M.Q, M.R_ORDER
(OP_FQ6_MUL, OP_FQ6_INV, OP_FQ6_MUL_BY_01, OP_FQ6_MUL_BY_1, OP_FQ12_MUL, OP_FQ12_SQR, OP_FQ12_INV, OP_FQ12_CONJUGATE, OP_FROB1, OP_FROB2, OP_FROB3,
 OP_MUL_BY_034, OP_FINAL_EXP) = range(13)
N_RANDOM = 256


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "pairing_golden.json")) as f:
        g = json.load(f)
    words = lambda h: np.array([int(x, 16) for x in h], dtype=np.uint64)  # noqa: E731
    entries = [("e_g1_g2", g1_raw(M.G1_GEN), g2_raw(M.G2_GEN), words(g["e_g1_g2"]))]
    for e in g["pairs"]:
        a, b = int(e["a"], 16), int(e["b"], 16)
        entries.append(("pair %x %x" % (a, b), g1_raw(M.ec_mul(M.FQ_OPS, M.G1_GEN, a)), g2_raw(M.ec_mul(M.FQ2_OPS, M.G2_GEN, b)), words(e["gt"])))
    for k, e in enumerate(g["jeff1"]):
        entries.append(("jeff1 %d" % k, words(e["g1"]), words(e["g2"]), words(e["gt"])))
    return entries


def g1_raw(p):
    return np.array(M.g1_affine_to_raw(p), dtype=np.uint64)


def g2_raw(p):
    return np.array(M.g2_affine_to_raw(p), dtype=np.uint64)


def ptr(a):
    return a.ctypes.data_as(C.c_void_p)


# ---------------------------------------------------------------- the model checks itself
def test_model_pairing_is_bilinear_and_has_order_r(golden):
    e = P.pairing(M.G1_GEN, M.G2_GEN)
    assert e != P.ONE
    assert P.f12_pow(e, R) == P.ONE
    e2 = P.f12_mul(e, e)
    assert P.pairing(M.ec_add(M.FQ_OPS, M.G1_GEN, M.G1_GEN), M.G2_GEN) == e2
    assert P.pairing(M.G1_GEN, M.ec_add(M.FQ2_OPS, M.G2_GEN, M.G2_GEN)) == e2
    # golden entries recomputed: e(G1, G2) and the two jeff1 pairs, whose product is one (EIP-197: the vector's expected output)
    assert P.gt_to_words(e) == golden[0][3].tolist()
    jeff = [P.pairing(M.g1_affine_from_raw(g1), M.g2_affine_from_raw(g2)) for name, g1, g2, _ in golden if name.startswith("jeff1")]
    assert [P.gt_to_words(v) for v in jeff] == [gt.tolist() for name, _, _, gt in golden if name.startswith("jeff1")]
    assert len(jeff) == 2 and P.f12_mul(jeff[0], jeff[1]) == P.ONE and jeff[0] != P.ONE


def test_model_tower_identities():
    rnd = random.Random(11)
    a = tuple((rnd.randrange(Q), rnd.randrange(Q)) for _ in range(6))
    assert P.f12_frobenius(a, 1) == P.f12_pow(a, Q)             # the closed form against plain powering
    assert P.f12_frobenius(a, 2) == P.f12_frobenius(P.f12_frobenius(a, 1), 1)
    assert P.f12_frobenius(a, 6) == P.f12_conjugate(a) and P.f12_frobenius(a, 12) == a
    assert P.f12_mul(a, P.f12_inv(a)) == P.ONE
    assert P.from_tower(P.to_tower(a)) == a and P.gt_from_words(P.gt_to_words(a)) == a
    w = (P.F2_ZERO, P.F2_ONE) + (P.F2_ZERO,) * 4
    w2 = P.f12_mul(w, w)
    assert w2 == P.fq6_embed((P.F2_ZERO, P.F2_ONE, P.F2_ZERO))   # w^2 = v
    assert P.f12_mul(P.f12_mul(w2, w2), w2) == (P.XI,) + (P.F2_ZERO,) * 5   # v^3 = xi
    # the arithmetic behind "no step of the loop meets T = +-Q": 6u + 2 + q - q^2 + q^3 = 0 mod r
    assert (P.ATE_LOOP + Q - Q * Q + Q ** 3) % R == 0


def test_constants_file_is_generated():
    import importlib.util

    spec = importlib.util.spec_from_file_location("gen_pairing_constants", os.path.join(ROOT, "tools", "gen_pairing_constants.py"))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    with open(os.path.join(ROOT, "phase2-bn254_amd", "csrc", "pairing_constants.inc")) as f:
        assert f.read() == gen.render(), "pairing_constants.inc is stale: run tools/gen_pairing_constants.py"


# ---------------------------------------------------------------- tower primitives against the model
def f2_words(x):
    return M.to_limbs(M.to_mont(x[0], Q)) + M.to_limbs(M.to_mont(x[1], Q))


def f6_words(c):
    return [w for x in c for w in f2_words(x)]


def f6_from_words(words):
    fq = [M.from_mont(M.from_limbs(words[4 * i:4 * i + 4]), Q) for i in range(6)]
    return tuple((fq[2 * i], fq[2 * i + 1]) for i in range(3))


def run_op(lib, op, operands, out_words):
    inp = np.array([w for o in operands for w in o], dtype=np.uint64)
    out = np.zeros(out_words, dtype=np.uint64)
    assert lib.mi355zk_selftest_pairing_op(op, ptr(inp), inp.size, ptr(out), out_words) == 0
    return [int(v) for v in out]


def rand_f2(rnd):
    return (rnd.randrange(Q), rnd.randrange(Q))


def rand_f6(rnd):
    return tuple(rand_f2(rnd) for _ in range(3))


def rand_f12(rnd):
    return tuple(rand_f2(rnd) for _ in range(6))


def edges(n_f2):
    """all coefficients 0, 1 and q - 1; one nonzero Fq coefficient (q - 1, then a full-width value) in each of the 2 n positions"""
    out = [tuple((v, v) for _ in range(n_f2)) for v in (0, 1, Q - 1)]
    for pos in range(2 * n_f2):
        for v in (Q - 1, 0x2A1908F7E6D5C4B3A29180706F5E4D3C2B1A091B7E4D3C2A190807F6E5D4C3B % Q):
            flat = [0] * (2 * n_f2)
            flat[pos] = v
            out.append(tuple((flat[2 * i], flat[2 * i + 1]) for i in range(n_f2)))
    return out


def f6_mul_model(a, b):
    return P.fq6_project(P.f12_mul(P.fq6_embed(a), P.fq6_embed(b)))


def f6_inv_model(a):
    if a == (P.F2_ZERO,) * 3:
        return a                                             # the library's convention: 1 / 0 = 0
    return P.fq6_project(P.f12_inv(P.fq6_embed(a)))


def f12_inv_model(a):
    return a if a == P.ZERO else P.f12_inv(a)


F6_ONE = (P.F2_ONE, P.F2_ZERO, P.F2_ZERO)


def test_fq6_ops(zk):
    lib = zk.lib.load()
    rnd = random.Random(2)
    E = edges(3)
    ops2 = [(rand_f6(rnd), rand_f6(rnd)) for _ in range(N_RANDOM)] + [(a, b) for a in E for b in E[:9]] + [(a, rand_f6(rnd)) for a in E]
    for a, b in ops2:
        assert run_op(lib, OP_FQ6_MUL, [f6_words(a), f6_words(b)], 24) == f6_words(f6_mul_model(a, b)), (a, b)
    for a in [rand_f6(rnd) for _ in range(N_RANDOM)] + E:
        got = run_op(lib, OP_FQ6_INV, [f6_words(a)], 24)
        assert got == f6_words(f6_inv_model(a)), a
        if any(x != P.F2_ZERO for x in a):                    # a * (1 / a) = 1, through the library's own product
            assert run_op(lib, OP_FQ6_MUL, [f6_words(a), got], 24) == f6_words(F6_ONE)
    for a in [rand_f6(rnd) for _ in range(N_RANDOM)] + E:
        b0, b1 = rand_f2(rnd), rand_f2(rnd)
        for c0, c1 in ((b0, b1), (P.F2_ZERO, b1), (b0, P.F2_ZERO), ((Q - 1, Q - 1), (Q - 1, Q - 1))):
            want = f6_words(f6_mul_model(a, (c0, c1, P.F2_ZERO)))
            assert run_op(lib, OP_FQ6_MUL_BY_01, [f6_words(a), f2_words(c0), f2_words(c1)], 24) == want
            assert run_op(lib, OP_FQ6_MUL, [f6_words(a), f6_words((c0, c1, P.F2_ZERO))], 24) == want   # sparse == dense
        assert run_op(lib, OP_FQ6_MUL_BY_1, [f6_words(a), f2_words(b1)], 24) == f6_words(f6_mul_model(a, (P.F2_ZERO, b1, P.F2_ZERO)))


def test_fq12_mul_sqr(zk):
    lib = zk.lib.load()
    rnd = random.Random(3)
    E = edges(6)
    W = P.gt_to_words
    for a, b in [(rand_f12(rnd), rand_f12(rnd)) for _ in range(N_RANDOM)] + [(a, b) for a in E for b in E[:5]] + [(rand_f12(rnd), b) for b in E]:
        assert run_op(lib, OP_FQ12_MUL, [W(P.from_tower(a)), W(P.from_tower(b))], 48) == W(P.f12_mul(P.from_tower(a), P.from_tower(b)))
    for a in [rand_f12(rnd) for _ in range(N_RANDOM)] + E:
        a = P.from_tower(a)
        assert run_op(lib, OP_FQ12_SQR, [W(a)], 48) == W(P.f12_sqr(a))


def test_fq12_inv_conjugate_frobenius(zk):
    lib = zk.lib.load()
    rnd = random.Random(4)
    W = P.gt_to_words
    for a in [rand_f12(rnd) for _ in range(N_RANDOM)] + edges(6):
        a = P.from_tower(a)
        got = run_op(lib, OP_FQ12_INV, [W(a)], 48)
        assert got == W(f12_inv_model(a))
        if a != P.ZERO:
            assert run_op(lib, OP_FQ12_MUL, [W(a), got], 48) == W(P.ONE)
        assert run_op(lib, OP_FQ12_CONJUGATE, [W(a)], 48) == W(P.f12_conjugate(a))
        for k, op in ((1, OP_FROB1), (2, OP_FROB2), (3, OP_FROB3)):
            assert run_op(lib, op, [W(a)], 48) == W(P.f12_frobenius(a, k)), k
    # frobenius^12 is the identity, as 12 x q, 6 x q^2, 4 x q^3
    for a in [rand_f12(rnd) for _ in range(8)] + edges(6)[:3]:
        for op, times in ((OP_FROB1, 12), (OP_FROB2, 6), (OP_FROB3, 4)):
            x = W(a)
            for _ in range(times):
                x = run_op(lib, op, [x], 48)
            assert x == W(a)


def test_fq12_mul_by_034(zk):
    lib = zk.lib.load()
    rnd = random.Random(5)
    W = P.gt_to_words
    lines = [(rand_f2(rnd), rand_f2(rnd), rand_f2(rnd)) for _ in range(4)]
    lines += [(P.F2_ZERO, P.F2_ZERO, P.F2_ZERO), (P.F2_ONE, P.F2_ZERO, P.F2_ZERO), ((Q - 1, Q - 1),) * 3, (P.F2_ZERO, rand_f2(rnd), P.F2_ZERO),
              (P.F2_ZERO, P.F2_ZERO, rand_f2(rnd)), ((rnd.randrange(Q), 0), rand_f2(rnd), rand_f2(rnd))]
    cases = [(P.from_tower(rand_f12(rnd)), (rand_f2(rnd), rand_f2(rnd), rand_f2(rnd))) for _ in range(N_RANDOM)]
    cases += [(P.from_tower(a), ln) for a in edges(6) for ln in lines[:3]] + [(P.from_tower(rand_f12(rnd)), ln) for ln in lines]
    for a, (c0, c3, c4) in cases:
        want = W(P.f12_mul(a, P.line_034(c0, c3, c4)))
        assert run_op(lib, OP_MUL_BY_034, [W(a), f2_words(c0), f2_words(c3), f2_words(c4)], 48) == want
        assert run_op(lib, OP_FQ12_MUL, [W(a), W(P.line_034(c0, c3, c4))], 48) == want     # the sparse product equals the dense one


def test_final_exponentiation_is_the_exact_exponent(zk):
    """the addition chain of the hard part against one square-and-multiply by (q^12 - 1) / r, on values that are NOT Miller values"""
    lib = zk.lib.load()
    rnd = random.Random(6)
    W = P.gt_to_words
    for a in [P.from_tower(rand_f12(rnd)) for _ in range(4)] + [P.ONE, P.from_tower(edges(6)[2])]:
        assert run_op(lib, OP_FINAL_EXP, [W(a)], 48) == W(P.final_exponentiation(a))


def test_selftest_op_rejects_bad_shapes(zk):
    lib = zk.lib.load()
    buf = np.zeros(96, dtype=np.uint64)
    out = np.zeros(48, dtype=np.uint64)
    for op, in_words, out_words in ((OP_FQ12_MUL, 48, 48), (OP_FQ12_MUL, 96, 24), (OP_FQ6_MUL, 96, 24), (OP_MUL_BY_034, 48, 48), (13, 48, 48), (-1, 48, 48)):
        assert lib.mi355zk_selftest_pairing_op(op, ptr(buf), in_words, ptr(out), out_words) == zk.lib.ERR_BAD_ARGS
    assert lib.mi355zk_selftest_pairing_op(OP_FQ12_SQR, None, 48, ptr(out), 48) == zk.lib.ERR_BAD_ARGS
    assert lib.mi355zk_selftest_pairing_op(OP_FQ12_SQR, ptr(buf), 48, None, 48) == zk.lib.ERR_BAD_ARGS


# ---------------------------------------------------------------- the host product
def product(lib, g1, g2):
    g1 = np.ascontiguousarray(np.asarray(g1, dtype=np.uint64).reshape(-1, 8))
    g2 = np.ascontiguousarray(np.asarray(g2, dtype=np.uint64).reshape(-1, 16))
    out = np.zeros(48, dtype=np.uint64)
    assert lib.mi355zk_bn254_pairing_product(ptr(out), ptr(g1), ptr(g2), g1.shape[0]) == 0
    return out


def test_host_product_matches_every_golden_entry(zk, golden):
    lib = zk.lib.load()
    for name, g1, g2, gt in golden:
        assert np.array_equal(product(lib, g1, g2), gt), name


def test_host_product_identities(zk, golden):
    lib = zk.lib.load()
    one = np.array(P.gt_to_words(P.ONE), dtype=np.uint64)
    assert np.array_equal(one, zk.pairing.GT_ONE)
    out = np.zeros(48, dtype=np.uint64)
    assert lib.mi355zk_bn254_pairing_product(ptr(out), None, None, 0) == 0 and np.array_equal(out, one)   # n = 0
    _, g1, g2, gt = golden[0]
    assert np.array_equal(product(lib, np.zeros(8, np.uint64), g2), one)                                  # zero P
    assert np.array_equal(product(lib, g1, np.zeros(16, np.uint64)), one)                                 # zero Q
    assert np.array_equal(product(lib, [g1, np.zeros(8, np.uint64), g1], [np.zeros(16, np.uint64), g2, g2]), gt)   # ... drop out of a product
    jeff = [(a, b) for name, a, b, _ in golden if name.startswith("jeff1")]
    assert np.array_equal(product(lib, [jeff[0][0], jeff[1][0]], [jeff[0][1], jeff[1][1]]), one)          # EIP-197: the product is one
    doubled = g1_raw(M.ec_add(M.FQ_OPS, *(M.g1_affine_from_raw(jeff[0][0]),) * 2))
    assert not np.array_equal(product(lib, [doubled, jeff[1][0]], [jeff[0][1], jeff[1][1]]), one)
    # bad arguments
    assert lib.mi355zk_bn254_pairing_product(None, ptr(g1), ptr(g2), 1) == zk.lib.ERR_BAD_ARGS
    assert lib.mi355zk_bn254_pairing_product(ptr(out), None, ptr(g2), 1) == zk.lib.ERR_BAD_ARGS
    assert lib.mi355zk_bn254_pairing_product(ptr(out), ptr(g1), None, 1) == zk.lib.ERR_BAD_ARGS
    assert lib.mi355zk_bn254_pairing_product(ptr(out), ptr(g1), ptr(g2), 1 << 31) == zk.lib.ERR_BAD_ARGS
    # the device entry points refuse bad arguments before they touch a device
    assert lib.mi355zk_bn254_pairing_product_dev(None, None, None, 4, None, 4, None) == zk.lib.ERR_BAD_ARGS
    assert lib.mi355zk_bn254_gt_is_one_dev(None, None, 4, None) == zk.lib.ERR_BAD_ARGS
    assert lib.mi355zk_bn254_gt_eq_dev(None, None, None, 4, None) == zk.lib.ERR_BAD_ARGS


# ---------------------------------------------------------------- the Python layer, host side
def test_python_layer_on_host_records(zk, golden):
    _, g1, g2, gt = golden[0]
    assert np.array_equal(zk.pairing.pairing(g1, g2), gt)
    x = 0x1F2E3D4C5B6A79880796A5B4C3D2E1F0
    xg1, xg2 = g1_raw(M.ec_mul(M.FQ_OPS, M.G1_GEN, x)), g2_raw(M.ec_mul(M.FQ2_OPS, M.G2_GEN, x))
    assert zk.pairing.same_ratio((g1, xg1), (g2, xg2))
    assert not zk.pairing.same_ratio((g1, xg1), (g2, g2_raw(M.ec_mul(M.FQ2_OPS, M.G2_GEN, x + 1))))
    for pos in range(4):
        pts = [g1, xg1, g2, xg2]
        pts[pos] = np.zeros_like(pts[pos])
        assert not zk.pairing.same_ratio((pts[0], pts[1]), (pts[2], pts[3]))
    # -(x, y): e(P, -Q) e(P, Q) = 1
    neg = zk.pairing._neg_record(g2)
    assert np.array_equal(neg, g2_raw(M.ec_neg(M.FQ2_OPS, M.G2_GEN)))
    assert np.array_equal(zk.pairing.miller_loop_product([(g1, g2), (g1, neg)]), zk.pairing.GT_ONE)


def test_verify_proof_length_check_needs_no_device(zk, golden):
    _, g1, g2, _ = golden[0]
    vk = {"alpha_g1": g1, "beta_g2": g2, "gamma_g2": g2, "delta_g2": g2, "ic": np.stack([g1, g1])}
    pvk = zk.pairing.prepare_verifying_key(vk)
    assert np.array_equal(pvk["alpha_g1_beta_g2"], golden[0][3]) and pvk["ic"].shape == (2, 8)
    for inputs in ([], [1, 2]):
        with pytest.raises(zk.SynthesisError) as e:
            zk.pairing.verify_proof(pvk, (g1, g2, g1), inputs)
        assert e.value.kind == zk.SynthesisError.MALFORMED_VERIFYING_KEY
    with pytest.raises(zk.SynthesisError):
        zk.pairing.verify_proofs(pvk, [(g1, g2, g1)] * 2, [[5], [5, 6]])
