"""The witness batch's host side (no GPU): the three new ABI symbols and their argument rules, the row predicate of the satisfaction
check (mi355zk_selftest_r1cs_check: the function the kernel runs, on host arrays) against big ints, circom.UnsatisfiedConstraint, and
the refusals of circom.prepare_provers_dev."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import r1cs_cases as K
import witness_cases as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mi355zk_bn254_fr_sparse_matvec_batch_dev", "mi355zk_bn254_fr_r1cs_check_dev", "mi355zk_selftest_r1cs_check")
r = K.R_ORDER


def _zk():
    import phase2_bn254_amd as zk

    return zk


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def test_the_three_symbols_are_declared_exported_and_bound():
    zk = _zk()
    header = open(os.path.join(ROOT, "include", "mi355zk.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    lib = zk.lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in zk.lib.SIGNATURES and hasattr(lib, name), name
    assert lib.mi355zk_abi_version() == 7 and zk.lib.ABI_VERSION == 7
    limit = int(re.search(r"#define\s+MI355ZK_R1CS_MAX_VECTORS\s+(\d+)", header).group(1))
    assert limit == zk.lib.R1CS_MAX_VECTORS and limit >= 4096
    rust = open(os.path.join(ROOT, "integration", "mi355zk.rs")).read()
    assert "pub fn mi355zk_bn254_fr_sparse_matvec_batch_dev(" in rust and "pub fn mi355zk_bn254_fr_r1cs_check_dev(" in rust
    assert "mi355zk_selftest_r1cs_check" not in rust


def test_the_batch_product_refuses_bad_arguments_without_a_device():
    zk = _zk()
    lib = zk.lib.load()
    BAD, LIMIT = zk.lib.ERR_BAD_ARGS, zk.lib.R1CS_MAX_VECTORS
    # host memory stands in for the device arrays: every call below is refused (or has nothing to do) before any device work
    buf = [np.zeros(4096, np.uint64) for _ in range(6)]
    out, rp, col, cid, cf, x = (_p(b) for b in buf)
    good = dict(out=out, out_stride=6, rp=rp, col=col, cid=cid, cf=cf, n_coeffs=2, x=x, n_x=3, x_stride=4, n_vectors=5, n_rows=4, nnz=5)

    def call(**kw):
        a = dict(good, **kw)
        return lib.mi355zk_bn254_fr_sparse_matvec_batch_dev(a["out"], a["out_stride"], a["rp"], a["col"], a["cid"], a["cf"], a["n_coeffs"], a["x"],
                                                            a["n_x"], a["x_stride"], a["n_vectors"], a["n_rows"], a["nnz"], None)

    for name in ("out", "rp", "col", "cid", "cf", "x"):                    # what the single call refuses: a NULL pointer with a count
        assert call(**{name: None}) == BAD, name
    for name in ("n_rows", "nnz", "n_x", "n_coeffs"):                      # ... a count >= 2^32
        for big in (1 << 32, (1 << 32) + 5, 1 << 40):
            assert call(**{name: big, "x_stride": 1 << 41, "out_stride": 1 << 41}) == BAD, (name, big)
    assert call(out=x) == BAD                                              # ... d_out == d_x
    assert call(n_vectors=0) == BAD
    assert call(n_vectors=LIMIT + 1) == BAD and call(n_vectors=1 << 40) == BAD
    assert call(x_stride=2) == BAD and call(x_stride=0) == BAD             # x_stride < n_x
    assert call(out_stride=3) == BAD and call(out_stride=0) == BAD         # out_stride < n_rows
    base = buf[5].ctypes.data
    x_bytes, out_bytes = (4 * 4 + 3) * 32, (4 * 6 + 4) * 32                # the two ranges of `good`
    for off in (32, x_bytes - 32, -32, -(out_bytes - 32)):                 # an out range that overlaps the x range, from either side
        assert call(out=C.c_void_p(base + 2048 * 8 + off), x=C.c_void_p(base + 2048 * 8)) == BAD, off
    assert call(out_stride=1 << 62, n_vectors=1 << 12) == BAD              # a range that does not fit the address space
    assert call(n_rows=0) == 0                                             # nothing to do: succeeds, launches nothing
    assert call(n_rows=0, out=None, out_stride=0, rp=None, nnz=0, col=None, cid=None) == 0
    assert call(n_rows=0, n_vectors=LIMIT, out=None, out_stride=0) == 0 and call(n_rows=0, n_vectors=1) == 0   # (the limit itself is allowed)
    assert call(n_rows=0, n_vectors=0) == BAD and call(n_rows=0, x_stride=2) == BAD   # the refusals come first


def test_the_check_call_refuses_bad_arguments_without_a_device():
    zk = _zk()
    lib = zk.lib.load()
    BAD, LIMIT = zk.lib.ERR_BAD_ARGS, zk.lib.R1CS_MAX_VECTORS
    a, b, c = (np.zeros(256, np.uint64) for _ in range(3))
    first, count = (C.c_longlong * 4)(7, 7, 7, 7), (C.c_uint32 * 4)(9, 9, 9, 9)
    good = dict(a=_p(a), b=_p(b), c=_p(c), n_rows=4, stride=6, n_vectors=3, first=first, count=count)

    def call(**kw):
        k = dict(good, **kw)
        return lib.mi355zk_bn254_fr_r1cs_check_dev(k["a"], k["b"], k["c"], k["n_rows"], k["stride"], k["n_vectors"], k["first"], k["count"], None)

    for name in ("a", "b", "c", "first"):                                  # a NULL array with n_rows > 0, a NULL first_bad
        assert call(**{name: None}) == BAD, name
    assert call(first=None, n_rows=0) == BAD
    assert call(n_vectors=0) == BAD and call(n_vectors=LIMIT + 1) == BAD
    assert call(stride=3) == BAD and call(stride=0) == BAD                 # vector_stride < n_rows
    for big in (1 << 32, (1 << 32) + 1, 1 << 40):
        assert call(n_rows=big, stride=1 << 41) == BAD, big
    assert list(first) == [7] * 4 and list(count) == [9] * 4               # a refused call writes nothing
    assert call(n_rows=0) == 0                                             # no rows: -1 / 0 for every vector, no device work
    assert list(first) == [-1, -1, -1, 7] and list(count) == [0, 0, 0, 9]
    first[0] = 5
    assert call(n_rows=0, a=None, b=None, c=None, stride=0, count=None, n_vectors=1) == 0 and first[0] == -1


def _selftest(zk, a, b, c):
    """mi355zk_selftest_r1cs_check on canonical ints -> (first, count)"""
    ma, mb, mc = K.mont(a), K.mont(b), K.mont(c)
    first, count = C.c_longlong(99), C.c_uint32(99)
    assert zk.lib.load().mi355zk_selftest_r1cs_check(_p(ma), _p(mb), _p(mc), len(a), C.byref(first), C.byref(count)) == 0
    return first.value, count.value


def test_the_row_predicate_against_big_ints():
    zk = _zk()
    rng = np.random.default_rng(5200)
    uni = lambda: int.from_bytes(rng.bytes(40), "little") % r  # noqa: E731
    x = uni()
    assert _selftest(zk, [r - 1], [r - 1], [1]) == (-1, 0)                 # (r - 1)(r - 1) = 1
    assert _selftest(zk, [r - 1], [r - 1], [2]) == (0, 1)
    assert _selftest(zk, [0, x], [x, 0], [0, 0]) == (-1, 0)                # 0 x = 0, x 0 = 0
    assert _selftest(zk, [x], [0], [5]) == (0, 1)                          # x 0 = c != 0
    assert _selftest(zk, [x], [0], [r - 1]) == (0, 1)
    assert _selftest(zk, [], [], []) == (-1, 0)
    # c differs from a b in ONE limb of its Montgomery form: the lowest, then the top one (a change that keeps the value below r)
    lib = zk.lib.load()
    seen = 0
    for _ in range(64):
        a, b = uni(), uni()
        ma, mb, good = K.mont([a]), K.mont([b]), K.mont([a * b])
        for word, bit in ((0, 0), (0, 63), (3, 0), (3, 58)):
            mc = good.copy()
            mc[0, word] ^= np.uint64(1 << bit)
            if K.from_limbs(mc)[0] >= r:
                continue                                                   # (not a canonical word: outside the contract)
            first, count = C.c_longlong(99), C.c_uint32(99)
            assert lib.mi355zk_selftest_r1cs_check(_p(ma), _p(mb), _p(mc), 1, C.byref(first), C.byref(count)) == 0
            assert (first.value, count.value) == (0, 1), (word, bit)
            seen += 1
        first = C.c_longlong(99)
        assert lib.mi355zk_selftest_r1cs_check(_p(ma), _p(mb), _p(good), 1, C.byref(first), None) == 0 and first.value == -1   # n_bad may be NULL
    assert seen > 200
    # 1000 uniform rows, failures planted at rows 0, 1, 511 and the last
    a, b = [uni() for _ in range(1000)], [uni() for _ in range(1000)]
    c = [p * q % r for p, q in zip(a, b)]
    assert _selftest(zk, a, b, c) == (-1, 0) == W.verdict(a, b, c)
    for planted in ([999], [511, 999], [1, 511, 999], [0, 1, 511, 999], [0], [1], [511]):
        bad = list(c)
        for i in planted:
            bad[i] = (bad[i] + 1 + i) % r
        assert _selftest(zk, a, b, bad) == (planted[0], len(planted)) == W.verdict(a, b, bad), planted
    assert lib.mi355zk_selftest_r1cs_check(None, None, None, 3, C.byref(C.c_longlong()), None) == zk.lib.ERR_BAD_ARGS
    assert lib.mi355zk_selftest_r1cs_check(_p(K.mont(a)), _p(K.mont(b)), _p(K.mont(c)), 3, None, None) == zk.lib.ERR_BAD_ARGS


def test_unsatisfied_constraint_is_a_synthesis_error():
    zk = _zk()
    assert zk.SynthesisError.UNSATISFIABLE == "Unsatisfiable"
    e = zk.circom.UnsatisfiedConstraint(2, 17, 3, 5, 6, 31)
    assert isinstance(e, zk.SynthesisError) and e.kind == "Unsatisfiable"
    assert (e.witness, e.index, e.count, e.a, e.b, e.c) == (2, 17, 3, 5, 6, 31)
    assert "Unsatisfiable" in str(e) and "witness 2" in str(e) and "constraint 17" in str(e) and "exponent" not in str(e)
    assert str(zk.SynthesisError("UnexpectedIdentity", 4)) == "UnexpectedIdentity at exponent 4"     # the other kinds keep their wording


def test_the_satisfied_circuit_is_satisfied_and_its_breakers_break_their_rows():
    zk = _zk()
    s = W.satisfied_circuit(zk)
    circuit = s.circuit
    assert circuit.witness[0] == 1 and len(circuit.witness) == circuit.num_inputs + circuit.num_aux
    assert W.failing_rows(circuit, circuit.witness) == []
    lens = {len(lc) for con in circuit.constraints for lc in con[:2]}
    assert 0 in lens and 70 in lens
    other = s.witness()
    assert other != circuit.witness and W.failing_rows(circuit, other) == []
    assert W.failing_rows(circuit, s.break_witness(other, [3, 250])) == [3, 250]
    assert W.failing_rows(s.break_coefficient(zk, [17]), circuit.witness) == [17]
    small = K.small_circuit(zk)
    assert W.failing_rows(small, small.witness) == []


def test_prepare_provers_dev_refuses_bad_witnesses_before_any_device_work():
    zk = _zk()
    circuit = K.small_circuit(zk)
    cc = zk.circom.CompiledCircuit(zk.circom._compile_host(circuit), "cpu")      # (host tensors: the refusals below come first)
    ints, good = list(circuit.witness), K.to_limbs(circuit.witness)
    with pytest.raises(ValueError, match="witness 1"):                           # a ragged list
        zk.circom.prepare_provers_dev(cc, [ints, ints[:-1], ints])
    with pytest.raises(ValueError, match="witness 2"):
        zk.circom.prepare_provers_dev(cc, [good, ints, good[:-1]])
    for bad in (np.stack([good, good])[:, :-1], np.stack([good, good])[:, :, :3], good):     # the array form: not (B, n_vars, 4)
        with pytest.raises(ValueError):
            zk.circom.prepare_provers_dev(cc, bad)
    for v in (r, r + 1, (1 << 256) - 1):                                         # a value >= r in witness k
        for k in (0, 2):
            batch = np.stack([good, good, good])
            batch[k, 4] = K.to_limbs([v])[0]
            with pytest.raises(ValueError, match="witness %d" % k):
                zk.circom.prepare_provers_dev(cc, batch)
            with pytest.raises(ValueError, match="witness %d" % k):
                zk.circom.prepare_provers_dev(cc, [batch[0], batch[1], batch[2]])
    with pytest.raises(ValueError):
        zk.circom.prepare_provers_dev(cc, [ints[:-1]], check=True)
    assert zk.circom.prepare_provers_dev(cc, []) == []
