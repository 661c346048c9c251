"""Batch inversion on the HOST (mi355zk_selftest_fr_batch_inverse: the lane routines of csrc/fr_inverse.hpp in the kernels' grouping into
runs, tiles, product trees and carry chunks, no device) against Python big ints, byte for byte and with the count of zeros, at every size
where the grouping changes; and the argument refusals of the device entry points."""
import ctypes as C

import numpy as np
import pytest

import fr_inverse_cases as V

FILL = 0xA5A5A5A5A5A5A5A5


@pytest.fixture(scope="module")
def lib(zk):
    return zk.lib.load()


def _inverse_host(lib, a: np.ndarray, in_place=False):
    n = a.shape[0]
    out = a.copy() if in_place else np.full((n, 4), FILL, np.uint64)
    src = out if in_place else a
    nz = C.c_uint32(0xFFFFFFFF)
    assert lib.mi355zk_selftest_fr_batch_inverse(out.ctypes.data_as(C.c_void_p) if n else None, src.ctypes.data_as(C.c_void_p) if n else None, n,
                                                 C.byref(nz)) == 0
    return out, nz.value


def test_geometry_is_powers_of_two(lib):
    run, tile, cw = V.geometry(lib)
    for v in (run, tile, cw):
        assert v >= 2 and v & (v - 1) == 0
    assert tile % run == 0
    assert lib.mi355zk_fr_inverse_geometry(None, None, None) == 3


@pytest.mark.parametrize("size_name", V.SIZE_NAMES)
def test_host_inversion_matches_big_ints(lib, size_name):
    geom = V.geometry(lib)
    n = V.size(size_name, geom)
    for pattern in V.PATTERNS:
        want, want_zeros = V.expected(pattern, n, geom)
        for in_place in (False, True):
            got, zeros = _inverse_host(lib, V.element_rows(pattern, n, geom), in_place)
            assert zeros == want_zeros, (pattern, n, in_place)
            assert np.array_equal(got, want), (pattern, n, in_place)


def test_host_inversion_across_a_carry_chunk(lib):
    """(carry_width + 1) tiles and one element: the second chunk of the launch that turns tile products into tile inverses"""
    geom = V.geometry(lib)
    n = V.size("largest", geom)
    want, want_zeros = V.expected("zero_at_tile_boundary", n, geom)
    got, zeros = _inverse_host(lib, V.element_rows("zero_at_tile_boundary", n, geom))
    assert zeros == want_zeros == 1 and np.array_equal(got, want)


def test_host_hook_refusals_and_no_counter(lib):
    a = V.element_rows("zero_first", 3, V.geometry(lib))
    out = np.zeros_like(a)
    assert lib.mi355zk_selftest_fr_batch_inverse(out.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), 3, None) == 0
    assert np.array_equal(out, V.expected("zero_first", 3, V.geometry(lib))[0])
    assert lib.mi355zk_selftest_fr_batch_inverse(None, a.ctypes.data_as(C.c_void_p), 3, None) == 3
    assert lib.mi355zk_selftest_fr_batch_inverse(out.ctypes.data_as(C.c_void_p), None, 3, None) == 3
    assert lib.mi355zk_selftest_fr_batch_inverse(out.ctypes.data_as(C.c_void_p), a.ctypes.data_as(C.c_void_p), 1 << 32, None) == 3


def test_device_entry_points_refuse_bad_arguments_without_a_device(lib, zk):
    """rc 3 before any device work: the pointers below are never dereferenced"""
    bad = zk.lib.ERR_BAD_ARGS
    inv, dv = lib.mi355zk_bn254_fr_batch_inverse_dev, lib.mi355zk_bn254_fr_evals_divide_dev
    a, b = 0x200000, 0x400000
    assert inv(None, C.c_void_p(a), 8, None, None) == bad
    assert inv(C.c_void_p(b), None, 8, None, None) == bad
    assert inv(C.c_void_p(b), C.c_void_p(a), 1 << 32, None, None) == bad
    assert inv(C.c_void_p(a + 32), C.c_void_p(a), 8, None, None) == bad        # partial overlap, out above in
    assert inv(C.c_void_p(a - 7 * 32), C.c_void_p(a), 8, None, None) == bad    # ... and below: the last element of out is the first of in
    z = np.concatenate([V.rows([3 * V.MONT % V.R])[0], V.rows([4 * V.MONT % V.R])[0]])
    zp, q, vals, ev = z.ctypes.data_as(C.c_void_p), C.c_void_p(0x800000), C.c_void_p(0x100000), C.c_void_p(a)
    assert dv(q, 8, None, ev, 3, zp, 1, None) == bad
    assert dv(q, 8, vals, None, 3, zp, 1, None) == bad
    assert dv(q, 8, vals, ev, 3, None, 1, None) == bad
    assert dv(q, 8, vals, ev, 29, zp, 1, None) == bad
    assert dv(q, 8, vals, ev, 3, zp, 0, None) == bad
    assert dv(q, 8, vals, ev, 3, zp, zk.lib.POLY_MAX_POINTS + 1, None) == bad
    assert dv(q, 7, vals, ev, 3, zp, 2, None) == bad                                   # q_stride < n
    assert dv(C.c_void_p(a + 32), 8, vals, ev, 3, zp, 1, None) == bad                 # q inside the evaluations
    assert dv(C.c_void_p(a - 9 * 32 - 32), 9, vals, ev, 3, zp, 2, None) == bad        # the second quotient reaches into them
    assert dv(C.c_void_p(0x100000 - 8 * 32 + 32), 8, vals, ev, 3, zp, 1, None) == bad  # the quotient's last element is values[0]
