"""mi355zk_bn254_fr_poly_divide_dev / _eval_dev (csrc/fr_poly.hip) against Python big ints -- kate_divison (sonic/util.rs:444-463) and a
Horner evaluation -- byte for byte: the grid of test_fr_poly_host.py on the device, several points per call, strided quotients, and one
size that crosses a chunk boundary of the carry kernel."""
import ctypes as C

import numpy as np
import pytest

import fr_poly_cases as P

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A5A5A5A5A


@pytest.fixture(scope="module")
def lib(zk, worker):
    return zk.lib.load()


def _zs(zs) -> np.ndarray:
    return np.concatenate([P.mont(z) for z in zs])


def _dev(a: np.ndarray):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def divide(lib, a: np.ndarray, zs, q_stride=None, with_rem=True):
    """-> (the whole (B, q_stride, 4) quotient buffer with its sentinels, (B, 4) remainders or None)"""
    import torch

    n, b = a.shape[0], len(zs)
    q_stride = max(n - 1, 0) if q_stride is None else q_stride
    q = torch.full((b, q_stride, 4), SENTINEL, dtype=torch.int64, device="cuda")
    rem = torch.full((b, 4), SENTINEL, dtype=torch.int64, device="cuda") if with_rem else None
    d_a, z = _dev(a), _zs(zs)
    rc = lib.mi355zk_bn254_fr_poly_divide_dev(C.c_void_p(q.data_ptr()) if q.numel() else None, q_stride, C.c_void_p(rem.data_ptr()) if with_rem else None,
                                              C.c_void_p(d_a.data_ptr()) if n else None, n, z.ctypes.data_as(C.c_void_p), b, None)
    assert rc == 0
    torch.cuda.synchronize()
    return _host(q), (_host(rem) if with_rem else None)


def evaluate(lib, a: np.ndarray, zs) -> np.ndarray:
    import torch

    out = torch.full((len(zs), 4), SENTINEL, dtype=torch.int64, device="cuda")
    d_a, z = _dev(a), _zs(zs)
    assert lib.mi355zk_bn254_fr_poly_eval_dev(C.c_void_p(out.data_ptr()), C.c_void_p(d_a.data_ptr()) if a.shape[0] else None, a.shape[0],
                                              z.ctypes.data_as(C.c_void_p), len(zs), None) == 0
    torch.cuda.synchronize()
    return _host(out)


def _check(lib, pattern, n, zs, coeff_z=0):
    a = P.coefficient_rows(pattern, n, coeff_z)
    q, rem = divide(lib, a, zs)
    ev = evaluate(lib, a, zs)
    for j, z in enumerate(zs):
        want_q, want_rem = P.expected(pattern, n, z)
        assert np.array_equal(rem[j], want_rem), (pattern, n, j, hex(z))
        assert np.array_equal(ev[j], rem[j]), (pattern, n, j, hex(z))
        assert np.array_equal(q[j], want_q), (pattern, n, j, hex(z))


@pytest.mark.parametrize("size_name", P.SIZE_NAMES)
def test_division_and_evaluation_match_big_ints(lib, size_name):
    """every coefficient pattern at every point: all the points in one call, except where the coefficients depend on the point"""
    geom = P.geometry(lib)
    n, zs = P.size(size_name, geom), P.points(geom)
    for pattern in P.PATTERNS:
        if pattern == "exact_multiple":
            for z in zs:
                _check(lib, pattern, n, [z], coeff_z=z)
        else:
            _check(lib, pattern, n, zs)


@pytest.mark.parametrize("b", [1, 2, 5])
def test_points_per_call_with_a_repeated_point(lib, b):
    geom = P.geometry(lib)
    base = P.points(geom)[4:] + [2]
    zs = base[:b - 1] + [base[0]] if b > 1 else base[:1]
    assert len(zs) == b
    _check(lib, "random", geom[1] + 1, zs)


def test_strided_quotients_leave_the_gaps_alone(lib):
    geom = P.geometry(lib)
    n, zs = geom[1] + 1, [P.Z_FIXED, 1, P.Z_FIXED]
    a = P.coefficient_rows("random", n, 0)
    q, rem = divide(lib, a, zs, q_stride=n + 3)
    for j, z in enumerate(zs):
        want_q, want_rem = P.expected("random", n, z)
        assert np.array_equal(q[j, :n - 1], want_q) and np.array_equal(rem[j], want_rem)
        assert (q[j, n - 1:].view(np.int64) == SENTINEL).all()


def test_no_remainder_pointer(lib):
    geom = P.geometry(lib)
    n = geom[0] + 1
    q, rem = divide(lib, P.coefficient_rows("random", n, 0), [P.Z_FIXED, 2], with_rem=False)
    assert rem is None
    for j, z in enumerate([P.Z_FIXED, 2]):
        assert np.array_equal(q[j], P.expected("random", n, z)[0])


def test_one_coefficient_and_none(lib):
    a = P.coefficient_rows("random", 1, 0)
    q, rem = divide(lib, a, [P.Z_FIXED, 0])
    assert q.size == 0 and np.array_equal(rem[0], a[0]) and np.array_equal(rem[1], a[0])
    assert np.array_equal(evaluate(lib, a, [P.Z_FIXED])[0], a[0])
    none = np.zeros((0, 4), np.uint64)
    q, rem = divide(lib, none, [P.Z_FIXED, 3])
    assert q.size == 0 and not rem.any()
    assert not evaluate(lib, none, [P.Z_FIXED, 3]).any()


def test_largest_size_crosses_a_carry_chunk(lib):
    """(carry_width + 1) tiles and one coefficient, two points in one call: the fixed point and an element of order TILE"""
    geom = P.geometry(lib)
    _check(lib, "random", P.size("largest", geom), P.points(geom)[4:][::2])
