"""mi355zk_bn254_fr_ratio_scan_dev (csrc/fr_scan.hip) against Python big ints, byte for byte: the scan of num[i] / den[i] over two rows, with
and without numerators, into the denominators' own array and into another, with zero denominators at a run boundary and at a tile boundary
(counted; their terms are zero); and against the three calls it fuses -- batch_inverse, mul_assign_dev, fr_scan_dev.  The reference inverts by
Montgomery's trick and checks itself against pow(., -1, r) on a sample (fr_inverse_cases.reference)."""
import ctypes as C

import numpy as np
import pytest

import fr_inverse_cases as I
import fr_scan_cases as V

pytestmark = pytest.mark.gpu
SENTINEL = 0x5A5A5A5A5A5A5A5A
GUARD = 5
SIZES = ("1", "run+1", "tile+1", "2tile+3")


@pytest.fixture(scope="module")
def lib(zk, worker):
    return zk.lib.load()


def _dev(a: np.ndarray):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def _vp(t):
    return C.c_void_p(t.data_ptr())


def _case(n, geom):
    """two rows of raw words: (numerators, denominators, the number of zero denominators); row 1 has zeros at the run and the tile boundary"""
    run, tile, _ = geom
    den = [list(V.elements("random", n, geom, 5000)), list(V.elements("random", n, geom, 6000))]
    zeros = sorted({min(run, n - 1), min(tile, n - 1)}) if n > 1 else []
    for i in zeros:
        den[1][i] = 0
    num = [list(V.elements("random", n, geom, 7000)), list(V.elements("random", n, geom, 8000))]
    return num, den, len(zeros)


def _reference(num, den, flags):
    """(outputs, total) of one row from its raw words"""
    inv = I.reference(den)                                       # raw words of 1 / den, zero for zero
    return V.reference(inv, num, flags)                          # the terms are num[i] inv[i], or inv[i]


def ratio(lib, num, den, flags, in_place):
    """-> ((2, n + GUARD, 4) outputs with their guards, (2, 4) totals, the count of zeros)"""
    import torch

    n = len(den[0])
    stride = n + GUARD
    host_den = np.full((2, stride, 4), SENTINEL, np.uint64)
    for r in range(2):
        host_den[r, :n] = V.rows(den[r])
    d_den = _dev(host_den)
    d_num = _dev(np.stack([V.rows(x) for x in num])) if num is not None else None
    out = d_den if in_place else torch.full((2, stride, 4), SENTINEL, dtype=torch.int64, device="cuda")
    total = torch.full((3, 4), SENTINEL, dtype=torch.int64, device="cuda")
    zeros = torch.full((1,), 0x7FFFFFFF, dtype=torch.int32, device="cuda")
    rc = lib.mi355zk_bn254_fr_ratio_scan_dev(_vp(out), stride, _vp(d_num) if num is not None else None, n, _vp(d_den), stride, n, 2, flags, _vp(total),
                                             _vp(zeros), None)
    assert rc == 0
    torch.cuda.synchronize()
    if not in_place:
        assert np.array_equal(_host(d_den), host_den)
    if num is not None:
        assert np.array_equal(_host(d_num), np.stack([V.rows(x) for x in num]))
    tot = _host(total)
    assert (tot[2].view(np.int64) == SENTINEL).all()
    return _host(out), tot[:2], int(zeros.item())


@pytest.mark.parametrize("size_name", SIZES)
def test_ratio_scan_matches_big_ints(lib, size_name):
    geom = V.geometry(lib)
    n = V.size(size_name, geom)
    num, den, n_zero = _case(n, geom)
    for flags in V.MODES:
        for with_num in (True, False):
            want = [_reference(num[r] if with_num else None, den[r], flags) for r in range(2)]
            for in_place in (False, True):
                out, total, zeros = ratio(lib, num if with_num else None, den, flags, in_place)
                what = (n, flags, with_num, in_place)
                assert zeros == n_zero, what
                for r in range(2):
                    assert np.array_equal(out[r, :n], V.rows(want[r][0])), what + (r,)
                    assert np.array_equal(total[r], V.rows([want[r][1]])[0]), what + (r,)
                    assert (out[r, n:].view(np.int64) == SENTINEL).all(), what + (r,)
    if n_zero:   # a product row is zero from its first zero denominator on; a sum row merely misses those terms
        first = min(i for i, d in enumerate(den[1]) if d == 0)
        prod, _ = _reference(num[1], den[1], 0)
        assert all(v == 0 for v in prod[first:]) and all(v != 0 for v in prod[:first])
        sums, _ = _reference(num[1], den[1], V.SUM)
        assert sums[first] == (sums[first - 1] if first else 0)


@pytest.mark.parametrize("size_name", SIZES)
def test_ratio_scan_equals_the_three_calls_it_fuses(lib, zk, size_name):
    import torch

    geom = V.geometry(lib)
    n = V.size(size_name, geom)
    num, den, n_zero = _case(n, geom)
    d_num = _dev(np.stack([V.rows(x) for x in num]))
    d_den = _dev(np.stack([V.rows(x) for x in den]))
    for flags in (V.EXCLUSIVE, V.SUM):
        terms, zeros = zk.kzg.batch_inverse(d_den, count_zeros=True)
        assert zeros == n_zero
        assert lib.mi355zk_bn254_fr_mul_assign_dev(_vp(terms), _vp(d_num), 2 * n, None) == 0
        want = torch.empty_like(terms)
        want_total = torch.empty((2, 4), dtype=torch.int64, device="cuda")
        assert lib.mi355zk_bn254_fr_scan_dev(_vp(want), n, _vp(terms), n, n, 2, flags, _vp(want_total), None) == 0
        f = zk.grand_product.ratio_sums if flags & V.SUM else zk.grand_product.ratio_products
        got, got_total, got_zeros = f(d_num, d_den, exclusive=bool(flags & V.EXCLUSIVE), total=True, allow_zero=True)
        assert got_zeros == n_zero
        assert torch.equal(got, want) and torch.equal(got_total, want_total)
        if n_zero:
            with pytest.raises(ZeroDivisionError, match=str(n_zero)):
                f(d_num, d_den)
        else:
            assert torch.equal(f(d_num, d_den, exclusive=bool(flags & V.EXCLUSIVE)), want)
    with pytest.raises(ValueError):
        zk.grand_product.ratio_products(d_num, d_den, out=d_num, allow_zero=True)      # out may not be num
    with pytest.raises(ValueError):
        zk.grand_product.ratio_products(d_num[:1], d_den, allow_zero=True)             # another shape


def test_refusals_and_the_cleared_counter(lib, zk):
    import torch

    bad = zk.lib.ERR_BAD_ARGS
    buf = torch.full((64, 4), SENTINEL, dtype=torch.int64, device="cuda")
    zeros = torch.full((1,), 77, dtype=torch.int32, device="cuda")
    f = lib.mi355zk_bn254_fr_ratio_scan_dev
    p = lambda i: C.c_void_p(buf.data_ptr() + 32 * i)  # noqa: E731
    z = _vp(zeros)
    assert f(None, 8, None, 8, p(0), 8, 8, 1, 0, None, z, None) == bad
    assert f(p(32), 8, None, 8, None, 8, 8, 1, 0, None, z, None) == bad
    assert f(p(32), 8, None, 8, p(0), 8, 1 << 32, 1, 0, None, z, None) == bad
    assert f(p(32), 8, None, 8, p(0), 8, 8, 65536, 0, None, z, None) == bad
    assert f(p(32), 7, None, 8, p(0), 8, 8, 2, 0, None, z, None) == bad
    assert f(p(32), 8, None, 8, p(0), 7, 8, 2, 0, None, z, None) == bad
    assert f(p(32), 8, p(16), 7, p(0), 8, 8, 2, 0, None, z, None) == bad
    assert f(p(32), 8, None, 8, p(0), 8, 8, 1, 4, None, z, None) == bad
    assert f(p(1), 8, None, 8, p(0), 8, 8, 1, 0, None, z, None) == bad          # out overlaps den without being den
    assert f(p(32), 8, p(32), 8, p(0), 8, 8, 1, 0, None, z, None) == bad        # out is num
    assert f(p(32), 8, p(39), 8, p(0), 8, 8, 1, 0, None, z, None) == bad        # num starts at out's last element
    torch.cuda.synchronize()
    assert int(zeros.item()) == 77                                              # a refused call does no device work at all
    assert f(None, 0, None, 0, None, 0, 0, 2, 0, None, z, None) == 0            # nothing to do, and the counter is cleared
    torch.cuda.synchronize()
    assert int(zeros.item()) == 0
    assert (_host(buf).view(np.int64) == SENTINEL).all()
