"""The fixed-base window program of csrc/fixed_base.hpp on the HOST (no GPU): the signed 8-bit recoding the kernels run, and k * P through
the same recoding, step program and addition routine (mi355zk_selftest_fixed_base_mul) against the oracle's scalar multiplication."""
import ctypes as C

import numpy as np
import pytest

import bn254_model as M
import fixed_base_cases as FB
import inputs
import oracle_lib as O


@pytest.fixture(scope="module")
def lib(zk):
    return zk.lib.load()


def _digits(lib, k: int):
    kk = np.array(M.to_limbs(k), dtype=np.uint64)
    d = np.zeros(32, np.int16)
    assert lib.mi355zk_selftest_fixed_base_digits(kk.ctypes.data_as(C.c_void_p), d.ctypes.data_as(C.c_void_p)) == 0
    return [int(x) for x in d]


def test_digits_recompose_the_scalar(lib):
    ks = FB.edge_scalars() + FB.ints(inputs.random_scalars(2000, seed=9100))
    for k in ks:
        d = _digits(lib, k)
        assert sum(dw << (8 * w) for w, dw in enumerate(d)) == k, hex(k)
        assert all(abs(dw) <= 128 for dw in d), hex(k)
        assert d[31] <= 49, hex(k)
    assert _digits(lib, 0) == [0] * 32
    assert max(_digits(lib, k)[31] for k in ks) >= 48 and any(128 in _digits(lib, k) for k in ks) and any(-127 in _digits(lib, k) for k in ks)


def test_digits_of_any_256_bits_stay_in_range(lib):
    """a scalar >= r may lose the carry out of window 31; its digits still index the table"""
    for k in (M.R_ORDER, (1 << 256) - 1, int("80" * 32, 16), int("81" * 32, 16)):
        assert all(-128 <= dw <= 128 for dw in _digits(lib, k))


def test_hooks_refuse_bad_arguments(lib):
    d = np.zeros(32, np.int16)
    k = np.zeros(4, np.uint64)
    out = np.zeros(16, np.uint64)
    assert lib.mi355zk_selftest_fixed_base_digits(None, d.ctypes.data_as(C.c_void_p)) == 3
    assert lib.mi355zk_selftest_fixed_base_mul(3, inputs.G1_GEN_RAW.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 3
    zero = np.zeros(8, np.uint64)   # the identity is no base for a table
    assert lib.mi355zk_selftest_fixed_base_mul(1, zero.ctypes.data_as(C.c_void_p), k.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)) == 3
    assert lib.mi355zk_fixed_base_table_bytes(1) == 4096 * 64 and lib.mi355zk_fixed_base_table_bytes(2) == 4096 * 128
    assert lib.mi355zk_fixed_base_table_bytes(0) == 0 and lib.mi355zk_fixed_base_table_bytes(3) == 0


@pytest.mark.parametrize("group", [1, 2])
def test_host_program_matches_the_oracle(lib, group):
    G = O.G1 if group == 1 else O.G2
    gen = inputs.G1_GEN_RAW if group == 1 else inputs.G2_GEN_RAW
    ks = FB.test_scalars(64, seed=9101 + group)
    other = G.mul_many_affine(gen, inputs.random_scalars(1, seed=9110 + group))[0]
    for base in (gen, other):
        base = np.ascontiguousarray(base)
        want = G.mul_many_affine(base, ks)
        for i in range(ks.shape[0]):
            got = np.zeros(G.aff, np.uint64)
            assert lib.mi355zk_selftest_fixed_base_mul(group, base.ctypes.data_as(C.c_void_p), np.ascontiguousarray(ks[i]).ctypes.data_as(C.c_void_p),
                                                       got.ctypes.data_as(C.c_void_p)) == 0
            assert np.array_equal(got, want[i]), (group, hex(FB.ints(ks[i])[0]))
