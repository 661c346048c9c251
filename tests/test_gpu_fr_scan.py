"""mi355zk_bn254_fr_scan_dev and mi355zk_bn254_fr_mul_add_dev (csrc/fr_scan.hip, csrc/field_ops.hip) against the serial chain in Python big
ints, byte for byte: the grid of test_fr_scan_host.py on the device -- every size where the grouping into runs, tiles and carry chunks changes,
every pattern, products and sums, inclusive and exclusive -- out of place (the input unchanged) and in place, with guard elements behind every
row, three rows with a stride, the total of every row, and the refusals."""
import ctypes as C

import numpy as np
import pytest

import fr_scan_cases as V

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


def _vp(t, offset_elems=0):
    return C.c_void_p(t.data_ptr() + 32 * offset_elems)


def scan(lib, inputs_, flags: int, in_place: bool, stride=None):
    """the rows of `inputs_` (each (n, 4)) at `stride` elements -> (the (rows * stride + GUARD, 4) output buffer, the (rows, 4) totals)"""
    import torch

    rows, n = len(inputs_), inputs_[0].shape[0]
    stride = n if stride is None else stride
    host_in = np.full((rows * stride + GUARD, 4), SENTINEL, np.uint64)
    for r, a in enumerate(inputs_):
        host_in[r * stride:r * stride + n] = a
    d_in = _dev(host_in)
    out = d_in.clone() if in_place else torch.full((rows * stride + GUARD, 4), SENTINEL, dtype=torch.int64, device="cuda")
    total = torch.full((rows + 1, 4), SENTINEL, dtype=torch.int64, device="cuda")
    src = out if in_place else d_in
    rc = lib.mi355zk_bn254_fr_scan_dev(_vp(out) if n else None, stride, _vp(src) if n else None, stride, n, rows, flags, _vp(total), None)
    assert rc == 0
    torch.cuda.synchronize()
    if not in_place:
        assert np.array_equal(_host(d_in), host_in)   # the input of an out-of-place call is not written
    tot = _host(total)
    assert (tot[rows:].view(np.int64) == SENTINEL).all()
    return _host(out), tot[:rows]


def _check_rows(lib, patterns, n, geom, flags, in_place, stride=None):
    out, total = scan(lib, [V.element_rows(p, n, geom) for p in patterns], flags, in_place, stride)
    stride = n if stride is None else stride
    for r, p in enumerate(patterns):
        want, want_total = V.expected(p, n, geom, flags)
        what = (p, n, flags, in_place, r)
        assert np.array_equal(out[r * stride:r * stride + n], want), what
        assert np.array_equal(total[r], want_total), what
        assert (out[r * stride + n:(r + 1) * stride].view(np.int64) == SENTINEL).all(), what   # the gap behind the row
    assert (out[len(patterns) * stride:].view(np.int64) == SENTINEL).all(), (patterns, n, flags, in_place)


@pytest.mark.parametrize("size_name", V.SIZE_NAMES)
def test_scan_matches_the_serial_chain(lib, size_name):
    geom = V.geometry(lib)
    n = V.size(size_name, geom)
    for pattern in V.PATTERNS:
        for flags in V.MODES:
            for in_place in (False, True):
                _check_rows(lib, [pattern], n, geom, flags, in_place)


@pytest.mark.parametrize("size_name", ["run+1", "tile", "tile+1", "2tile+3"])
def test_three_rows_with_a_stride(lib, size_name):
    """row r at r * (n + 5) elements: the gaps are neither read into the chains nor written"""
    geom = V.geometry(lib)
    n = V.size(size_name, geom)
    for flags in V.MODES:
        for in_place in (False, True):
            _check_rows(lib, ["random", "zero_at_run_boundary", "zero_in_last_tile"], n, geom, flags, in_place, stride=n + 5)


def test_largest_size_crosses_a_carry_chunk(lib):
    """(carry_width + 1) tiles and one element: the carry launch walks two chunks of tile aggregates"""
    geom = V.geometry(lib)
    _check_rows(lib, ["zero_in_last_tile"], V.size("largest", geom), geom, V.EXCLUSIVE, True)


def test_empty_rows_fill_the_totals(lib):
    import torch

    one = V.rows([V.MONT])[0]
    for flags, want in ((0, one), (V.SUM, np.zeros(4, np.uint64))):
        total = torch.full((4, 4), SENTINEL, dtype=torch.int64, device="cuda")
        assert lib.mi355zk_bn254_fr_scan_dev(None, 0, None, 0, 0, 3, flags, _vp(total), None) == 0
        torch.cuda.synchronize()
        got = _host(total)
        assert (got[:3] == want).all() and (got[3].view(np.int64) == SENTINEL).all()
    total = torch.full((2, 4), SENTINEL, dtype=torch.int64, device="cuda")
    assert lib.mi355zk_bn254_fr_scan_dev(None, 0, None, 0, 8, 0, 0, _vp(total), None) == 0   # no rows: nothing at all
    torch.cuda.synchronize()
    assert (_host(total).view(np.int64) == SENTINEL).all()


def test_refusals_leave_the_buffers_untouched(lib, zk):
    import torch

    bad = zk.lib.ERR_BAD_ARGS
    buf = torch.full((64, 4), SENTINEL, dtype=torch.int64, device="cuda")
    f = lib.mi355zk_bn254_fr_scan_dev
    a, b, t = _vp(buf), _vp(buf, 32), _vp(buf, 60)
    assert f(None, 8, a, 8, 8, 1, 0, None, None) == bad
    assert f(b, 8, None, 8, 8, 1, 0, None, None) == bad
    assert f(b, 8, a, 8, 1 << 32, 1, 0, None, None) == bad
    assert f(b, 8, a, 8, 8, 65536, 0, None, None) == bad
    assert f(b, 7, a, 8, 8, 2, 0, None, None) == bad                    # out_stride < n with two rows
    assert f(b, 8, a, 7, 8, 2, 0, None, None) == bad                    # in_stride < n with two rows
    assert f(b, 8, a, 8, 8, 1, 4, None, None) == bad                    # an unknown flag bit
    assert f(_vp(buf, 1), 8, a, 8, 8, 1, 0, None, None) == bad          # out one element above in
    assert f(a, 8, _vp(buf, 7), 8, 8, 1, 0, None, None) == bad          # out's last element is in's first
    assert f(a, 8, a, 9, 8, 2, 0, None, None) == bad                    # in place with different strides
    assert f(a, 8, _vp(buf, 12), 8, 8, 2, 0, None, None) == bad         # the second row of out reaches the first of in
    assert f(b, 8, a, 8, 8, 2, 0, _vp(buf, 47), None) == bad            # the totals inside the outputs
    assert f(b, 8, a, 8, 8, 2, 0, _vp(buf, 15), None) == bad            # ... and inside the inputs
    assert f(b, 8, a, 8, 8, 2, 0, t, None) == 0                         # (the same call with the totals clear of both runs)
    torch.cuda.synchronize()
    got = _host(buf).view(np.int64)
    assert (got[:32] == SENTINEL).all() and (got[48:60] == SENTINEL).all() and (got[62:] == SENTINEL).all()
    with pytest.raises(ValueError):
        zk.grand_product.prefix_products(buf[:, :3])
    with pytest.raises(ValueError):
        zk.grand_product.prefix_products(buf[:8], out=buf[4:12])
    with pytest.raises(ValueError):
        zk.grand_product.prefix_sums(buf[:8], out=buf[:9])


def test_python_layer_shapes_and_totals(lib, zk):
    geom = V.geometry(lib)
    n = geom[1] + 1
    pats = ("random", "zero_last")
    a = _dev(np.stack([V.element_rows(p, n, geom) for p in pats]))
    out, tot = zk.grand_product.prefix_products(a, total=True)
    assert out.shape == (2, n, 4) and tot.shape == (2, 4)
    for r, p in enumerate(pats):
        want, want_total = V.expected(p, n, geom, 0)
        assert np.array_equal(_host(out[r]), want) and np.array_equal(_host(tot[r]), want_total)
    row = a[0].clone()
    same = zk.grand_product.prefix_sums(row, exclusive=True, out=row)       # in place, one row
    assert same is row and np.array_equal(_host(row), V.expected("random", n, geom, V.SUM | V.EXCLUSIVE)[0])
    wide = a.new_full((2, n + 3, 4), SENTINEL)
    zk.grand_product.prefix_products(a, out=wide[:, 1:n + 1])                # a strided view as the destination
    got = _host(wide)
    assert np.array_equal(got[:, 1:n + 1], _host(out)) and (got[:, 0].view(np.int64) == SENTINEL).all() and (got[:, n + 1:].view(np.int64) == SENTINEL).all()


@pytest.mark.parametrize("n_name", ["0", "1", "255", "256", "257", "2tile+3"])
def test_mul_add_matches_big_ints(lib, zk, n_name):
    import torch

    geom = V.geometry(lib)
    n = V.size(n_name, geom) if n_name == "2tile+3" else int(n_name)
    a, b = V.elements("random", n, geom), V.numerators(n, geom)
    rnd = 0x1234567 * V.MONT2 % V.R
    for c in (0, V.MONT, V.R - 1, rnd):          # raw words of 0, 1, a value with every limb set, and an arbitrary one
        cw = V.rows([c])
        for with_b in (True, False):
            buf = torch.full((n + GUARD, 4), SENTINEL, dtype=torch.int64, device="cuda")
            if n:
                buf[:n] = _dev(V.rows(a))
            d_b = _dev(V.rows(b)) if n else None
            rc = lib.mi355zk_bn254_fr_mul_add_dev(_vp(buf) if n else None, _vp(d_b) if (n and with_b) else None, cw.ctypes.data_as(C.c_void_p), n, None)
            assert rc == 0
            torch.cuda.synchronize()
            want = [(x + (V.mont_mul(c, y) if with_b else c)) % V.R for x, y in zip(a, b)]
            got = _host(buf)
            assert V.ints(got[:n]) == want, (n, c, with_b)
            assert (got[n:].view(np.int64) == SENTINEL).all()
            if n and with_b:
                assert np.array_equal(_host(d_b), V.rows(b))
    if n:   # the Python layer takes the scalar as an int mod r
        t = _dev(V.rows(a))
        assert zk.grand_product.mul_add(t, _dev(V.rows(b)), 5) is t
        assert V.ints(_host(t)) == [(x + 5 * y) % V.R for x, y in zip(a, b)]
        zk.grand_product.mul_add(t, None, V.R - 1)
        assert V.ints(_host(t)) == [(x + 5 * y + (V.R - 1) * V.MONT) % V.R for x, y in zip(a, b)]
