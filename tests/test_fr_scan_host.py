"""Prefix scans on the HOST (mi355zk_selftest_fr_scan: the lane routines of csrc/fr_scan.hpp in the kernels' grouping into runs, tiles and
carry chunks, no device) against the serial chain in Python big ints, byte for byte and with the total, at every size where the grouping
changes; the geometry, the ABI revision, the bindings, and the argument refusals of the device entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import fr_scan_cases as V

FILL = 0xA5A5A5A5A5A5A5A5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mi355zk_bn254_fr_scan_dev", "mi355zk_bn254_fr_ratio_scan_dev", "mi355zk_bn254_fr_mul_add_dev", "mi355zk_selftest_fr_scan",
           "mi355zk_fr_scan_geometry")


@pytest.fixture(scope="module")
def lib(zk):
    return zk.lib.load()


def _ptr(a):
    return a.ctypes.data_as(C.c_void_p) if a is not None and a.shape[0] else None


def _scan_host(lib, a: np.ndarray, num, flags: int, in_place=False):
    n = a.shape[0]
    out = a.copy() if in_place else np.full((n, 4), FILL, np.uint64)
    src = out if in_place else a
    total = np.full(4, FILL, np.uint64)
    assert lib.mi355zk_selftest_fr_scan(_ptr(out), _ptr(src), _ptr(num), n, flags, total.ctypes.data_as(C.c_void_p)) == 0
    return out, total


def test_geometry_is_powers_of_two(lib):
    run, tile, cw = V.geometry(lib)
    for v in (run, tile, cw):
        assert v >= 2 and v & (v - 1) == 0
    assert tile % run == 0
    assert lib.mi355zk_fr_scan_geometry(None, None, None) == 3


def test_abi_revision_and_bindings(lib, zk):
    assert lib.mi355zk_abi_version() == zk.lib.ABI_VERSION == 7   # symbols were added, no prototype changed
    rs = open(os.path.join(ROOT, "integration", "mi355zk.rs")).read()
    hdr = open(os.path.join(ROOT, "include", "mi355zk.h")).read()
    for name in SYMBOLS:
        assert name in zk.lib.SIGNATURES and hasattr(lib, name)
        assert re.search(r"\b%s\(" % name, hdr)
        # the generated extern block holds every public prototype; the self-test hooks stay out of it (tools/gen_rust_ffi.py)
        assert bool(re.search(r"pub fn %s\(" % name, rs)) == (not name.startswith("mi355zk_selftest_")), name
    assert (zk.lib.SCAN_SUM, zk.lib.SCAN_EXCLUSIVE) == (V.SUM, V.EXCLUSIVE)
    assert re.search(r"#define MI355ZK_SCAN_SUM\s+1u", hdr) and re.search(r"#define MI355ZK_SCAN_EXCLUSIVE\s+2u", hdr)


@pytest.mark.parametrize("size_name", V.SIZE_NAMES)
def test_host_scan_matches_the_serial_chain(lib, size_name):
    geom = V.geometry(lib)
    n = V.size(size_name, geom)
    num = V.numerator_rows(n, geom)
    for pattern in V.PATTERNS:
        a = V.element_rows(pattern, n, geom)
        for flags in V.MODES:
            for with_num in (False, True):
                want, want_total = V.expected(pattern, n, geom, flags, with_num)
                for in_place in (False, True):
                    got, total = _scan_host(lib, a, num if with_num else None, flags, in_place)
                    assert np.array_equal(got, want), (pattern, n, flags, with_num, in_place)
                    assert np.array_equal(total, want_total), (pattern, n, flags, with_num, in_place)


def test_host_scan_across_a_carry_chunk(lib):
    """(carry_width + 1) tiles and one element: the carry launch walks a second chunk"""
    geom = V.geometry(lib)
    n = V.size("largest", geom)
    a = V.element_rows("zero_in_last_tile", n, geom)
    for flags in (0, V.SUM | V.EXCLUSIVE):
        want, want_total = V.expected("zero_in_last_tile", n, geom, flags)
        got, total = _scan_host(lib, a, None, flags)
        assert np.array_equal(got, want) and np.array_equal(total, want_total), flags
    assert not V.expected("zero_in_last_tile", n, geom, 0)[1].any()   # the zero reaches the product's total


def test_host_hook_refusals_and_no_total(lib):
    geom = V.geometry(lib)
    a = V.element_rows("random", 3, geom)
    out = np.zeros_like(a)
    assert lib.mi355zk_selftest_fr_scan(_ptr(out), _ptr(a), None, 3, 0, None) == 0
    assert np.array_equal(out, V.expected("random", 3, geom, 0)[0])
    assert lib.mi355zk_selftest_fr_scan(None, _ptr(a), None, 3, 0, None) == 3
    assert lib.mi355zk_selftest_fr_scan(_ptr(out), None, None, 3, 0, None) == 3
    assert lib.mi355zk_selftest_fr_scan(_ptr(out), _ptr(a), None, 1 << 32, 0, None) == 3
    assert lib.mi355zk_selftest_fr_scan(_ptr(out), _ptr(a), None, 3, 4, None) == 3


def test_device_entry_points_refuse_bad_arguments_without_a_device(lib, zk):
    """rc 3 before any device work: the pointers below are never dereferenced"""
    bad = zk.lib.ERR_BAD_ARGS
    scan, ratio, mul_add = lib.mi355zk_bn254_fr_scan_dev, lib.mi355zk_bn254_fr_ratio_scan_dev, lib.mi355zk_bn254_fr_mul_add_dev
    a, b, t = 0x200000, 0x400000, 0x600000
    vp = C.c_void_p
    assert scan(None, 8, vp(a), 8, 8, 1, 0, None, None) == bad
    assert scan(vp(b), 8, None, 8, 8, 1, 0, None, None) == bad
    assert scan(vp(b), 8, vp(a), 8, 1 << 32, 1, 0, None, None) == bad
    assert scan(vp(b), 8, vp(a), 8, 8, 65536, 0, None, None) == bad
    assert scan(vp(b), 7, vp(a), 8, 8, 2, 0, None, None) == bad                 # out_stride < n with two rows
    assert scan(vp(b), 8, vp(a), 7, 8, 2, 0, None, None) == bad                 # in_stride < n with two rows
    assert scan(vp(b), 8, vp(a), 8, 8, 1, 4, None, None) == bad                 # an unknown flag bit
    assert scan(vp(a + 32), 8, vp(a), 8, 8, 1, 0, None, None) == bad            # partial overlap, out above in
    assert scan(vp(a - 7 * 32), 8, vp(a), 8, 8, 1, 0, None, None) == bad        # ... and below: the last element of out is the first of in
    assert scan(vp(a), 8, vp(a), 9, 8, 2, 0, None, None) == bad                 # in place with different strides
    assert scan(vp(b), 8, vp(a), 8, 8, 2, 0, vp(b + 15 * 32), None) == bad      # the totals inside the outputs
    assert scan(vp(b), 8, vp(a), 8, 8, 2, 0, vp(a - 32), None) == bad           # ... and reaching into the inputs
    assert ratio(None, 8, None, 8, vp(a), 8, 8, 1, 0, None, None, None) == bad
    assert ratio(vp(b), 8, None, 8, None, 8, 8, 1, 0, None, None, None) == bad
    assert ratio(vp(b), 8, None, 8, vp(a), 8, 1 << 32, 1, 0, None, None, None) == bad
    assert ratio(vp(b), 8, None, 8, vp(a), 8, 8, 65536, 0, None, None, None) == bad
    assert ratio(vp(b), 7, None, 8, vp(a), 8, 8, 2, 0, None, None, None) == bad
    assert ratio(vp(b), 8, None, 8, vp(a), 7, 8, 2, 0, None, None, None) == bad
    assert ratio(vp(b), 8, vp(t), 7, vp(a), 8, 8, 2, 0, None, None, None) == bad   # num_stride < n
    assert ratio(vp(b), 8, None, 8, vp(a), 8, 8, 1, 8, None, None, None) == bad
    assert ratio(vp(a + 32), 8, None, 8, vp(a), 8, 8, 1, 0, None, None, None) == bad   # out overlaps den without being den
    assert ratio(vp(b), 8, vp(b), 8, vp(a), 8, 8, 1, 0, None, None, None) == bad       # out is num
    assert ratio(vp(b), 8, vp(b + 7 * 32), 8, vp(a), 8, 8, 1, 0, None, None, None) == bad
    c = V.rows([V.MONT])
    assert mul_add(None, None, c.ctypes.data_as(vp), 4, None) == bad
    assert mul_add(vp(a), vp(b), None, 4, None) == bad
