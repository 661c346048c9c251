"""Division of an Fr polynomial by (x - z) on the HOST (mi355zk_selftest_fr_poly_divide: the kernels' routines of csrc/fr_poly.hpp in the
kernels' grouping into runs, tiles and carry chunks, no device) against Python big ints -- kate_divison (sonic/util.rs:444-463) and a Horner
evaluation -- byte for byte, at every size where the grouping changes; and the argument refusals of the two device entry points."""
import ctypes as C

import numpy as np
import pytest

import fr_poly_cases as P


@pytest.fixture(scope="module")
def lib(zk):
    return zk.lib.load()


def _divide_host(lib, a: np.ndarray, z: int):
    n = a.shape[0]
    q, rem = np.full((max(n - 1, 0), 4), 0xA5A5A5A5A5A5A5A5, np.uint64), np.zeros(4, np.uint64)
    assert lib.mi355zk_selftest_fr_poly_divide(q.ctypes.data_as(C.c_void_p) if n > 1 else None, rem.ctypes.data_as(C.c_void_p),
                                               a.ctypes.data_as(C.c_void_p), n, P.mont(z).ctypes.data_as(C.c_void_p)) == 0
    return q, rem


def test_geometry_is_powers_of_two(lib):
    run, tile, cw = P.geometry(lib)
    for v in (run, tile, cw):
        assert v >= 2 and v & (v - 1) == 0
    assert tile % run == 0
    assert lib.mi355zk_fr_poly_geometry(None, None, None) == 3


@pytest.mark.parametrize("size_name", P.SIZE_NAMES)
def test_host_division_matches_big_ints(lib, size_name):
    geom = P.geometry(lib)
    n = P.size(size_name, geom)
    for pattern in P.PATTERNS:
        for z in P.points(geom):
            q, rem = _divide_host(lib, P.coefficient_rows(pattern, n, z), z)
            want_q, want_rem = P.expected(pattern, n, z)
            assert np.array_equal(rem, want_rem), (pattern, n, hex(z))
            assert np.array_equal(q, want_q), (pattern, n, hex(z))


def test_host_division_across_a_carry_chunk(lib):
    """(carry_width + 1) tiles and one coefficient: the carry kernel's second chunk; random coefficients at the fixed point and at an
    element of order TILE (every tile multiplier is one)"""
    geom = P.geometry(lib)
    n = P.size("largest", geom)
    for z in P.points(geom)[4:][::2]:
        q, rem = _divide_host(lib, P.coefficient_rows("random", n, z), z)
        want_q, want_rem = P.expected("random", n, z)
        assert np.array_equal(rem, want_rem) and np.array_equal(q, want_q), hex(z)


def test_host_division_of_nothing(lib):
    rem = np.ones(4, np.uint64)
    assert lib.mi355zk_selftest_fr_poly_divide(None, rem.ctypes.data_as(C.c_void_p), None, 0, P.mont(5).ctypes.data_as(C.c_void_p)) == 0
    assert not rem.any()
    assert lib.mi355zk_selftest_fr_poly_divide(None, rem.ctypes.data_as(C.c_void_p), None, 3, P.mont(5).ctypes.data_as(C.c_void_p)) == 3


def test_device_entry_points_refuse_bad_arguments_without_a_device(lib, zk):
    """rc 3 before any device work: the pointers below are never dereferenced"""
    bad = zk.lib.ERR_BAD_ARGS
    z = np.concatenate([P.mont(3), P.mont(4)])
    zp, out, co, q = z.ctypes.data_as(C.c_void_p), C.c_void_p(0x100000), C.c_void_p(0x200000), C.c_void_p(0x400000)
    ev, dv = lib.mi355zk_bn254_fr_poly_eval_dev, lib.mi355zk_bn254_fr_poly_divide_dev
    assert ev(None, co, 8, zp, 1, None) == bad
    assert ev(out, None, 8, zp, 1, None) == bad
    assert ev(out, co, 8, None, 1, None) == bad
    assert ev(out, co, 1 << 32, zp, 1, None) == bad
    assert ev(out, co, 8, zp, 0, None) == bad
    assert ev(out, co, 8, zp, zk.lib.POLY_MAX_POINTS + 1, None) == bad
    assert dv(None, 7, out, co, 8, zp, 1, None) == bad
    assert dv(q, 7, out, None, 8, zp, 1, None) == bad
    assert dv(q, 7, out, co, 8, None, 1, None) == bad
    assert dv(q, 7, out, co, 1 << 32, zp, 1, None) == bad
    assert dv(q, 7, out, co, 8, zp, 0, None) == bad
    assert dv(q, 7, out, co, 8, zp, zk.lib.POLY_MAX_POINTS + 1, None) == bad
    assert dv(q, 6, out, co, 8, zp, 2, None) == bad                                   # q_stride < n - 1
    assert dv(C.c_void_p(0x200000 + 32), 7, out, co, 8, zp, 1, None) == bad           # q inside the coefficients
    assert dv(C.c_void_p(0x200000 - 7 * 32 - 32), 8, out, co, 8, zp, 2, None) == bad  # the second quotient reaches into them
