"""The prover's H-polynomial chain (bellman/src/groth16/prover.rs:216-248) in one call, on the GPU:
  - the fused elementwise kernel (mi355zk_bn254_fr_h_combine_dev) against big integers and against the three entry points it replaces;
  - the device-resident chain (mi355zk_bn254_fr_h_poly_dev) byte for byte against the ORACLE chain: oracle_lib.fr_domain_op for the seven
    transforms, oracle_lib.fe_mul_many for the two products, the subtraction mod r on the Montgomery forms (a - c commutes with the factor
    2^256), truncation;
  - the host-buffer entry (mi355zk_bn254_fr_h_poly): full and ragged lengths, inputs untouched, inputs at offsets of one larger buffer,
    four host threads at once;
  - the Python bindings (EvaluationDomain.h_poly, h_poly_host)."""
import ctypes as C
import threading

import numpy as np
import pytest

import bn254_model as M
import inputs
import oracle_lib as O

pytestmark = pytest.mark.gpu
R = M.R_ORDER
R_LIMBS = np.array(M.to_limbs(R), dtype=np.uint64)
INTO_REPR = 1


# ---------------------------------------------------------------------------------------------- reference side
def ints(x):
    return [M.from_limbs(row) for row in np.asarray(x, dtype=np.uint64).reshape(-1, 4).tolist()]


def limbs(vals):
    return np.array([M.to_limbs(v) for v in vals], dtype=np.uint64).reshape(-1, 4)


def sub_mod_r(x, y):
    """(x - y) mod r on (n, 4) u64 limbs of values < r: the limb-wise form of Python's (x - y) % R (test_sub_mod_r_helper holds it to that)"""
    x, y = np.asarray(x, dtype=np.uint64).reshape(-1, 4), np.asarray(y, dtype=np.uint64).reshape(-1, 4)
    out = np.empty_like(x)
    borrow = np.zeros(x.shape[0], dtype=np.uint64)
    for l in range(4):
        t = x[:, l] - y[:, l]
        b1 = x[:, l] < y[:, l]
        b2 = t < borrow
        out[:, l] = t - borrow
        borrow = (b1 | b2).astype(np.uint64)
    neg = borrow.astype(bool)
    carry = np.zeros(x.shape[0], dtype=np.uint64)
    for l in range(4):
        add = np.where(neg, R_LIMBS[l], np.uint64(0)).astype(np.uint64)
        t = out[:, l] + add
        c1 = t < add
        t2 = t + carry
        c2 = t2 < carry
        out[:, l] = t2
        carry = (c1 | c2).astype(np.uint64)
    return out


def zinv_mont(log_n):
    """Montgomery form of (7^(2^log_n) - 1)^-1 (divide_by_z_on_coset, domain.rs:217-234)"""
    z = (pow(M.FR_GENERATOR, 1 << log_n, R) - 1) % R
    return M.to_mont(pow(z, R - 2, R), R)


def oracle_h(a, b, c, log_n, into_repr=False):
    """the chain of prover.rs:216-248 through the oracle; a, b, c: (2^log_n, 4) Montgomery limbs -> (2^log_n - 1, 4)"""
    n = 1 << log_n
    ev = [O.fr_domain_op(O.fr_domain_op(x, log_n, "ifft"), log_n, "coset_fft").reshape(-1, 4) for x in (a, b, c)]
    t = sub_mod_r(O.fe_mul_many(O.FR, ev[0], ev[1]).reshape(-1, 4), ev[2])
    zi = np.tile(np.array(M.to_limbs(zinv_mont(log_n)), dtype=np.uint64), (n, 1))
    t = O.fe_mul_many(O.FR, t, zi).reshape(-1, 4)
    h = O.fr_domain_op(t, log_n, "icoset_fft").reshape(-1, 4)
    if into_repr:
        h = to_canonical_many(h)
    return h[:n - 1]


def to_canonical_many(x):
    """fe_to_canonical of every row: the Montgomery product with the plain integer 1 is x * 2^-256, i.e. into_repr, in one oracle call;
    a sample of rows is held to oracle_lib.fe_to_canonical itself"""
    x = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, 4)
    one = np.zeros_like(x)
    one[:, 0] = 1
    out = O.fe_mul_many(O.FR, x, one).reshape(-1, 4)
    for i in sorted({0, x.shape[0] // 2, x.shape[0] - 1} | set(range(0, x.shape[0], max(1, x.shape[0] // 61)))):
        assert np.array_equal(out[i], O.fe_to_canonical(O.FR, x[i])), i
    return out


def test_sub_mod_r_helper():
    rows = [0, 1, R - 1, R - 2, 1 << 64, (1 << 64) - 1, 1 << 128, (1 << 192) - 1, M.to_mont(1, R)] + ints(inputs.random_fr_mont(40, seed=11))
    xs = [x for x in rows for _ in rows]
    ys = [y for _ in rows for y in rows]
    assert ints(sub_mod_r(limbs(xs), limbs(ys))) == [(x - y) % R for x, y in zip(xs, ys)]


# ---------------------------------------------------------------------------------------------- device side
def dev(x):
    import torch

    return torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint64).view(np.int64)).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64).reshape(-1, 4)


def ptr(t):
    return C.c_void_p(t.data_ptr())


def sync():
    import torch

    torch.cuda.synchronize()


def combine(L, a, b, c, log_n):
    da, db, dc = dev(a), dev(b), dev(c)
    assert L.mi355zk_bn254_fr_h_combine_dev(ptr(da), ptr(db), ptr(dc), a.shape[0], log_n, None) == 0
    sync()
    assert np.array_equal(host(db), b) and np.array_equal(host(dc), c)   # b and c are only read
    return host(da)


def three_passes(L, a, b, c, log_n):
    """mul_assign, sub_assign, divide_by_z_on_coset: the sequence h_combine replaces (divide_by_z works on 2^log_n elements)"""
    da, db, dc = dev(a), dev(b), dev(c)
    n = a.shape[0]
    assert L.mi355zk_bn254_fr_mul_assign_dev(ptr(da), ptr(db), n, None) == 0
    assert L.mi355zk_bn254_fr_sub_assign_dev(ptr(da), ptr(dc), n, None) == 0
    assert n == 1 << log_n
    assert L.mi355zk_bn254_fr_divide_by_z_on_coset_dev(ptr(da), log_n, None) == 0
    sync()
    return host(da)


def model_combine(a, b, c, log_n):
    rinv, zi = pow(M.MONT_R, R - 2, R), zinv_mont(log_n)
    return [((x * y * rinv - z) % R) * zi * rinv % R for x, y, z in zip(ints(a), ints(b), ints(c))]


def edge_rows(seed=21):
    """(name, a, b, c) Montgomery forms as integers < r"""
    rinv = pow(M.MONT_R, R - 2, R)
    one = M.to_mont(1, R)
    rnd = ints(inputs.random_fr_mont(8, seed=seed))
    mm = lambda x, y: x * y * rinv % R   # noqa: E731
    rows = [
        ("a*b == c (random)", rnd[0], rnd[1], mm(rnd[0], rnd[1])),
        ("a*b == c (r-1 squared)", R - 1, R - 1, mm(R - 1, R - 1)),
        ("a*b == c (one, x)", one, rnd[2], rnd[2]),
        ("a == 0", 0, rnd[3], rnd[4]),
        ("b == 0", rnd[3], 0, rnd[4]),
        ("c == 0", rnd[3], rnd[4], 0),
        ("a == b == c == 0", 0, 0, 0),
        ("a == b == 0, c == r-1", 0, 0, R - 1),
        ("all r-1", R - 1, R - 1, R - 1),
        ("a == r-1", R - 1, rnd[5], rnd[6]),
        ("c == r-1", rnd[5], rnd[6], R - 1),
        ("all mont(1)", one, one, one),
        ("a == mont(1)", one, rnd[7], rnd[0]),
        ("c == mont(1)", rnd[1], rnd[2], one),
        ("a*b == 0 - c wraps: c == 1", rnd[3], rnd[5], 1),
    ]
    return rows


def test_h_combine_edge_rows_vs_big_integers(zk, worker):
    L = zk.lib.load()
    rows = edge_rows()
    a, b, c = (limbs([r[k] for r in rows]) for k in (1, 2, 3))
    for log_n in (0, 1, 4, 20, 28):
        got = ints(combine(L, a, b, c, log_n))
        want = model_combine(a, b, c, log_n)
        for r, g, w in zip(rows, got, want):
            assert g == w, (r[0], log_n)
        assert got[0] == got[1] == got[2] == 0   # a*b == c: the zero result, as the all-zero limbs
    # one row at a time (n = 1: a single lane of a single workgroup does the work)
    for r in rows:
        x, y, z = (limbs([r[k]]) for k in (1, 2, 3))
        assert ints(combine(L, x, y, z, 5)) == model_combine(x, y, z, 5), r[0]


GRID = 16384 * 256   # the launch is capped at 16384 workgroups of 256 lanes: longer arrays take the grid-stride loop


@pytest.mark.parametrize("n", [1, 255, 256, 257, GRID + 77])
def test_h_combine_lengths_vs_big_integers(zk, worker, n):
    L = zk.lib.load()
    rows = edge_rows(seed=22)
    log_n = 13   # (only selects z: n is free)
    a, b, c = (inputs.random_fr_mont(n, seed=400 + k).copy() for k in (0, 1, 2))
    m = min(n, len(rows))
    for k, arr in ((1, a), (2, b), (3, c)):
        arr[:m] = limbs([r[k] for r in rows[:m]])
    got = combine(L, a, b, c, log_n)
    # big integers: every element up to 2^12, beyond that the head, the tail (the second trip of the grid-stride loop) and a stride
    idx = np.arange(n) if n <= 4096 else np.unique(np.concatenate([np.arange(2048), np.arange(n - 2048, n), np.arange(GRID - 64, GRID + 64), np.arange(0, n, 4099)]))
    assert ints(got[idx]) == model_combine(a[idx], b[idx], c[idx], log_n)
    # and the whole array against the three kernels it replaces, which need n == 2^log_n only for the divide: use their own z
    da, db, dc = dev(a), dev(b), dev(c)
    assert L.mi355zk_bn254_fr_mul_assign_dev(ptr(da), ptr(db), n, None) == 0
    assert L.mi355zk_bn254_fr_sub_assign_dev(ptr(da), ptr(dc), n, None) == 0
    dz = dev(np.tile(np.array(M.to_limbs(zinv_mont(log_n)), dtype=np.uint64), (n, 1)))
    assert L.mi355zk_bn254_fr_mul_assign_dev(ptr(da), ptr(dz), n, None) == 0
    sync()
    assert np.array_equal(got, host(da))


@pytest.mark.parametrize("log_n", [0, 3, 8, 16, 20])
def test_h_combine_is_the_three_entry_points_in_sequence(zk, worker, log_n):
    L = zk.lib.load()
    n = 1 << log_n
    a, b, c = (inputs.random_fr_mont(n, seed=500 + 3 * log_n + k).copy() for k in (0, 1, 2))
    rows = edge_rows(seed=23)
    m = min(n, len(rows))
    for k, arr in ((1, a), (2, b), (3, c)):
        arr[:m] = limbs([r[k] for r in rows[:m]])
    assert np.array_equal(combine(L, a, b, c, log_n), three_passes(L, a, b, c, log_n))


def abc(log_n, seed, n=None):
    n = (1 << log_n) if n is None else n
    return tuple(inputs.random_fr_mont(n, seed=seed + k) for k in (0, 1, 2))


def h_poly_dev(L, a, b, c, log_n, flags):
    da, db, dc = dev(a), dev(b), dev(c)
    assert L.mi355zk_bn254_fr_h_poly_dev(ptr(da), ptr(db), ptr(dc), log_n, flags, None) == 0
    sync()
    return host(da)


@pytest.mark.parametrize("log_n", [0, 1, 2, 5, 10, 13, 16, 20])
def test_device_chain_matches_the_oracle_chain(zk, worker, log_n):
    L = zk.lib.load()
    n = 1 << log_n
    a, b, c = abc(log_n, 600 + 10 * log_n)
    want = oracle_h(a, b, c, log_n)
    got = h_poly_dev(L, a, b, c, log_n, 0)
    assert got.shape == (n, 4) and np.array_equal(got[:n - 1], want)
    got_repr = h_poly_dev(L, a, b, c, log_n, INTO_REPR)
    assert np.array_equal(got_repr[:n - 1], to_canonical_many(want) if n > 1 else want)
    assert np.array_equal(got_repr, to_canonical_many(got))   # every element is converted, the last one too


def test_device_chain_at_2_22_is_the_composed_chain(zk, worker):
    """2^22 has no full twiddle table (two passes of long rows, one transform per launch): held against the existing entry points"""
    import torch

    log_n = 22
    a, b, c = abc(log_n, 700)
    doms = [zk.EvaluationDomain(dev(x).view(-1, 4), log_n) for x in (a, b, c)]
    zk.EvaluationDomain.ifft_many(worker, doms)
    zk.EvaluationDomain.coset_fft_many(worker, doms)
    doms[0].mul_assign(worker, doms[1])
    doms[0].sub_assign(worker, doms[2])
    doms[0].divide_by_z_on_coset(worker)
    doms[0].icoset_fft(worker)
    torch.cuda.synchronize()
    want = host(doms[0].coeffs)
    del doms
    assert np.array_equal(h_poly_dev(zk.lib.load(), a, b, c, log_n, 0), want)


# ---------------------------------------------------------------------------------------------- host-buffer entry
def h_poly_host_raw(L, a, b, c, log_n, flags=0):
    """straight through the C entry: a, b, c may be views at offsets of a larger buffer (C-contiguous rows)"""
    n = 1 << log_n
    for x in (a, b, c):
        assert x.flags["C_CONTIGUOUS"] and x.dtype == np.uint64
    h = np.full((max(n - 1, 1), 4), 0xA5A5A5A5A5A5A5A5, dtype=np.uint64)
    p = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    rc = L.mi355zk_bn254_fr_h_poly(p(h), p(a), p(b), p(c), a.shape[0], log_n, flags)
    assert rc == 0, rc
    return h[:n - 1] if n > 1 else h


@pytest.mark.parametrize("log_n", [1, 12, 16])
def test_host_entry_full_length(zk, worker, log_n):
    L = zk.lib.load()
    a, b, c = abc(log_n, 800 + log_n)
    keep = [x.copy() for x in (a, b, c)]
    want = oracle_h(a, b, c, log_n)
    assert np.array_equal(h_poly_host_raw(L, a, b, c, log_n), want)
    assert all(np.array_equal(x, k) for x, k in zip((a, b, c), keep))   # a, b and c are never written
    assert np.array_equal(h_poly_host_raw(L, a, b, c, log_n, INTO_REPR), to_canonical_many(want))


def test_host_entry_log_n_zero_writes_nothing(zk, worker):
    L = zk.lib.load()
    a, b, c = abc(0, 810)
    h = h_poly_host_raw(L, a, b, c, 0)
    assert (h == 0xA5A5A5A5A5A5A5A5).all()   # 2^0 - 1 = no element, and the call succeeded


@pytest.mark.parametrize("length", [(1 << 12) - 37, (1 << 11) + 1, 1])
def test_host_entry_ragged_length_is_zero_padded(zk, worker, length):
    L = zk.lib.load()
    log_n = 12
    a, b, c = abc(log_n, 820, n=length)
    keep = [x.copy() for x in (a, b, c)]
    pad = lambda x: np.concatenate([x, np.zeros(((1 << log_n) - length, 4), np.uint64)])   # noqa: E731
    # a first call leaves non-zero data in the leased device buffer: the padding must be written, not inherited
    h_poly_host_raw(L, *abc(log_n, 830), log_n)
    got = h_poly_host_raw(L, a, b, c, log_n)
    assert np.array_equal(got, oracle_h(pad(a), pad(b), pad(c), log_n))
    assert all(np.array_equal(x, k) for x, k in zip((a, b, c), keep))


def test_host_entry_inputs_at_offsets_of_one_buffer(zk, worker):
    L = zk.lib.load()
    log_n, length = 12, (1 << 12) - 5
    big = inputs.random_fr_mont(4 * (1 << log_n), seed=840)
    keep = big.copy()
    # c before a before b, gaps between them, none at the start of the buffer
    c, a, b = big[3:3 + length], big[5000:5000 + length], big[10001:10001 + length]
    pad = lambda x: np.concatenate([x, np.zeros(((1 << log_n) - length, 4), np.uint64)])   # noqa: E731
    got = h_poly_host_raw(L, a, b, c, log_n)
    assert np.array_equal(got, oracle_h(pad(a), pad(b), pad(c), log_n))
    assert np.array_equal(big, keep)


def test_host_entry_from_four_threads(zk, worker):
    import torch

    L = zk.lib.load()
    log_n = 14
    ins = [abc(log_n, 900 + 10 * t) for t in range(4)]
    single = [h_poly_host_raw(L, *x, log_n) for x in ins]
    assert np.array_equal(single[0], oracle_h(*ins[0], log_n))
    assert not np.array_equal(single[0], single[1])
    out, errs = [None] * 4, []
    start = threading.Barrier(4)

    def run(t):
        try:
            torch.cuda.set_device(0)
            start.wait()
            for _ in range(3):
                out[t] = h_poly_host_raw(L, *ins[t], log_n)
                assert np.array_equal(out[t], single[t])
        except BaseException as e:  # noqa: BLE001
            errs.append((t, repr(e)))

    th = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    assert all(np.array_equal(o, s) for o, s in zip(out, single))


# ---------------------------------------------------------------------------------------------- Python bindings
@pytest.mark.parametrize("into_repr", [False, True])
def test_python_bindings_agree_with_each_other_and_the_oracle(zk, worker, into_repr):
    import torch

    log_n = 10
    n = 1 << log_n
    a, b, c = abc(log_n, 950)
    want = oracle_h(a, b, c, log_n, into_repr=into_repr)
    doms = [zk.EvaluationDomain.from_coeffs(dev(x).view(-1, 4)) for x in (a, b, c)]
    res = zk.EvaluationDomain.h_poly(doms[0], doms[1], doms[2], worker, into_repr=into_repr)
    torch.cuda.synchronize()
    assert res is doms[0]
    got_dev = host(res.into_coeffs())[:n - 1]
    got_host = zk.h_poly_host(a, b, c, log_n, into_repr=into_repr)
    assert got_host.shape == (n - 1, 4)
    assert np.array_equal(got_dev, want) and np.array_equal(got_host, want)
    # ragged input through the binding: from_coeffs pads on the device side, h_poly_host lets the library pad
    m = n - 100
    doms = [zk.EvaluationDomain.from_coeffs(dev(x[:m]).view(-1, 4)) for x in (a, b, c)]
    res = zk.EvaluationDomain.h_poly(doms[0], doms[1], doms[2], worker, into_repr=into_repr)
    torch.cuda.synchronize()
    assert np.array_equal(host(res.into_coeffs())[:n - 1], zk.h_poly_host(a[:m], b[:m], c[:m], log_n, into_repr=into_repr))
