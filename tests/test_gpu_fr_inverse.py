"""mi355zk_bn254_fr_batch_inverse_dev (csrc/fr_inverse.hip) against Python big ints, byte for byte: the grid of test_fr_inverse_host.py on
the device -- every size where the grouping into runs, tiles and carry chunks changes, every pattern of zeros -- out of place and in place,
with and without the counter of zeros, with guard elements behind the vector; the product a * (1 / a) through mul_assign_dev; the refusals."""
import ctypes as C

import numpy as np
import pytest

import fr_inverse_cases as V

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A5A5A5A5A
GUARD = 5


@pytest.fixture(scope="module")
def lib(zk, worker):
    return zk.lib.load()


def _dev(a: np.ndarray):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def inverse(lib, a: np.ndarray, in_place: bool, count: bool):
    """-> (the (n + GUARD, 4) output buffer with its guard elements, the counter or None)"""
    import torch

    n = a.shape[0]
    out = torch.full((n + GUARD, 4), SENTINEL, dtype=torch.int64, device="cuda")
    d_in = _dev(a)
    if in_place:
        out[:n] = d_in
    zeros = torch.full((1,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    src = out if in_place else d_in
    rc = lib.mi355zk_bn254_fr_batch_inverse_dev(C.c_void_p(out.data_ptr()) if n else None, C.c_void_p(src.data_ptr()) if n else None, n,
                                                C.c_void_p(zeros.data_ptr()) if count else None, None)
    assert rc == 0
    torch.cuda.synchronize()
    if not in_place and n:
        assert np.array_equal(_host(d_in), a)   # the input of an out-of-place call is not written
    return _host(out), (int(zeros.item()) if count else None)


def _check(lib, pattern, n, geom, modes=((False, False), (False, True), (True, False), (True, True))):
    a = V.element_rows(pattern, n, geom)
    want, want_zeros = V.expected(pattern, n, geom)
    for in_place, count in modes:
        out, zeros = inverse(lib, a, in_place, count)
        assert zeros == (want_zeros if count else None), (pattern, n, in_place)
        assert np.array_equal(out[:n], want), (pattern, n, in_place, count)
        assert (out[n:].view(np.int64) == SENTINEL).all(), (pattern, n, in_place, count)


@pytest.mark.parametrize("size_name", V.SIZE_NAMES)
def test_inversion_matches_big_ints(lib, size_name):
    geom = V.geometry(lib)
    n = V.size(size_name, geom)
    for pattern in V.PATTERNS:
        _check(lib, pattern, n, geom)


def test_largest_size_crosses_a_carry_chunk(lib):
    """(carry_width + 1) tiles and one element: the second launch walks two chunks of tile products"""
    geom = V.geometry(lib)
    _check(lib, "zero_at_tile_boundary", V.size("largest", geom), geom, modes=((True, True),))


def test_product_with_the_inverse_is_one(lib, zk):
    import torch

    geom = V.geometry(lib)
    n = 2 * geom[1] + 3
    a = _dev(V.element_rows("every_second_zero", n, geom))
    inv, zeros = zk.kzg.batch_inverse(a.reshape(1, n, 4), count_zeros=True)
    assert inv.shape == (1, n, 4) and zeros == (n + 1) // 2
    prod = a.clone()
    assert lib.mi355zk_bn254_fr_mul_assign_dev(C.c_void_p(prod.data_ptr()), C.c_void_p(inv.data_ptr()), n, None) == 0
    torch.cuda.synchronize()
    one = V.rows([V.MONT])[0]
    got = _host(prod)
    assert not got[0::2].any() and (got[1::2] == one).all()
    again = zk.kzg.batch_inverse(inv.reshape(n, 4))          # 1 / (1 / a) = a, zeros included
    assert np.array_equal(_host(again), _host(a))
    same = zk.kzg.batch_inverse(again, out=again)            # in place through the Python layer
    assert same is again and np.array_equal(_host(same), _host(inv).reshape(n, 4))


def test_refusals(lib, zk):
    import torch

    bad = zk.lib.ERR_BAD_ARGS
    buf = torch.full((24, 4), SENTINEL, dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    f = lib.mi355zk_bn254_fr_batch_inverse_dev
    assert f(C.c_void_p(p + 32), C.c_void_p(p), 8, None, None) == bad           # out one element above in
    assert f(C.c_void_p(p), C.c_void_p(p + 7 * 32), 8, None, None) == bad       # out's last element is in's first
    assert f(None, C.c_void_p(p), 8, None, None) == bad
    assert f(C.c_void_p(p), None, 8, None, None) == bad
    assert f(C.c_void_p(p), C.c_void_p(p + 8 * 32), 1 << 32, None, None) == bad
    zeros = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    assert f(None, None, 0, C.c_void_p(zeros.data_ptr()), None) == 0            # nothing to do, and the counter is cleared
    torch.cuda.synchronize()
    assert int(zeros.item()) == 0
    assert (_host(buf).view(np.int64) == SENTINEL).all()
    with pytest.raises(ValueError):
        zk.kzg.batch_inverse(buf[:, :3])
    with pytest.raises(ValueError):
        zk.kzg.batch_inverse(buf[:8], out=buf[4:12])
