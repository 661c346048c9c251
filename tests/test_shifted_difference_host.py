"""mi355zk_selftest_g1_shifted_difference: the lane routine of the H-bases kernel (csrc/point_diff.hip) run on the host, with the kernel's
grouping into shared inversions, against the integers (tests/bn254_model.py): out[i] = in[i + shift] - in[i] for small multiples of the
generator, every branch of the routine inside one shared inversion, groups that are all one exceptional case, group boundaries, and the
argument refusals of the device entry point (which need no device)."""
import ctypes as C

import numpy as np
import pytest

import bn254_model as M
import prepare_phase2_cases as P


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _host(zk, points: np.ndarray, shift: int, n_out: int) -> np.ndarray:
    out = np.full((n_out, 8), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    rc = zk.lib.load().mi355zk_selftest_g1_shifted_difference(_p(out), _p(points), points.shape[0], shift, n_out)
    assert rc == 0
    return out


def test_the_group_size_is_the_headers(zk):
    import os

    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi355zk.h")).read()
    assert "#define MI355ZK_SHIFTED_DIFFERENCE_K %d\n" % zk.lib.SHIFTED_DIFFERENCE_K in header
    assert P.K == zk.lib.SHIFTED_DIFFERENCE_K


@pytest.mark.parametrize("case", P.CASES, ids=P.CASE_IDS)
def test_host_twin_matches_the_integers(zk, case):
    _, multiples, shift, n_out = case
    points = P.raw(multiples)
    want = P.expected(multiples, shift, n_out)
    assert all(M.on_curve_g1(M.g1_affine_from_raw(r)) for r in want)
    assert np.array_equal(_host(zk, points, shift, n_out), want)


def test_the_first_case_holds_every_branch():
    """generic, equal, opposite (a doubling), left / right / both infinite: all within the first K outputs of the first case"""
    _, multiples, shift, n_out = P.CASES[0]
    assert n_out == P.K
    kinds = set()
    for i in range(n_out):
        a, b = multiples[i], multiples[i + shift]
        kinds.add("both" if a == 0 == b else "left" if a == 0 else "right" if b == 0 else "equal" if a == b else "opposite" if a == -b else "generic")
    assert kinds == {"both", "left", "right", "equal", "opposite", "generic"}


def test_a_doubling_is_the_doubling(zk):
    """in[i + shift] == -in[i]: 2 * in[i + shift], checked against the model's doubling and not only the table"""
    p = P.small_multiple(-4)
    want = np.array(M.g1_affine_to_raw(M.ec_add(M.FQ_OPS, p, p)), dtype=np.uint64)
    assert np.array_equal(_host(zk, P.raw([4, -4]), 1, 1)[0], want)


def test_bad_arguments(zk):
    L = zk.lib.load()
    bad = zk.lib.ERR_BAD_ARGS
    pts = P.raw(list(range(1, 9)))
    out = np.zeros((8, 8), dtype=np.uint64)
    for fn, tail in ((L.mi355zk_selftest_g1_shifted_difference, ()), (L.mi355zk_bn254_g1_shifted_difference_dev, (None,))):
        assert fn(_p(out), _p(pts), 8, 0, 4, *tail) == bad                 # shift == 0
        assert fn(_p(out), _p(pts), 8, 5, 4, *tail) == bad                 # shift + n_out > n_in
        assert fn(_p(out), _p(pts), 8, 9, 0, *tail) == bad                 # shift > n_in
        assert fn(_p(out), _p(pts), 8, (1 << 64) - 2, 4, *tail) == bad     # shift + n_out wraps
        assert fn(None, _p(pts), 8, 4, 4, *tail) == bad
        assert fn(_p(out), None, 8, 4, 4, *tail) == bad
        assert fn(_p(pts), _p(pts), 8, 4, 4, *tail) == bad                 # out == in
        assert fn(C.c_void_p(pts.ctypes.data + 7 * 64), _p(pts), 8, 4, 4, *tail) == bad   # out starts inside in
        assert fn(C.c_void_p(pts.ctypes.data + 64), _p(pts), 8, 4, 4, *tail) == bad
        assert fn(None, None, 8, 4, 0, *tail) == 0                        # n_out == 0: a valid no-op
    assert L.mi355zk_bn254_g1_shifted_difference_dev(C.c_void_p(out.ctypes.data + 8), _p(pts), 8, 4, 4, None) == bad   # not 16-byte aligned
    # the input may lie directly behind the output
    both = np.zeros((12, 8), dtype=np.uint64)
    both[4:] = pts
    assert L.mi355zk_selftest_g1_shifted_difference(_p(both), C.c_void_p(both.ctypes.data + 4 * 64), 8, 4, 4) == 0
    assert np.array_equal(both[:4], P.expected(list(range(1, 9)), 4, 4))
