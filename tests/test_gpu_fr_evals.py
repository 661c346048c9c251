"""mi355zk_bn254_fr_evals_divide_dev (csrc/fr_evals.hip): values and quotients of a polynomial given by its evaluations over the domain,
byte for byte against the coefficient route it replaces -- kzg.evaluate(ifft(evals)) and the fft of kzg.divide(ifft(evals)) padded with one
zero -- and, up to 2^5 points, against kate_divison in Python big ints.  Points outside the domain, every kind of point inside it, and an
element of order 2 n (z^n = -1); 1, 3 and 65 points per call; values only; strided quotients; the refusals."""
import ctypes as C
import functools

import numpy as np
import pytest

import bn254_model as M
import fr_inverse_cases as V
import fr_poly_cases as P
import inputs

pytestmark = pytest.mark.gpu
R = M.R_ORDER
SENTINEL = 0x5A5A5A5A5A5A5A5A
LOG_NAMES = ("0", "1", "2", "log_run", "log_tile", "log_tile+1")


@pytest.fixture(scope="module")
def lib(zk, worker):
    return zk.lib.load()


def _dev(a: np.ndarray):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def log_n_of(name: str, lib) -> int:
    run, tile, _ = V.geometry(lib)
    return {"0": 0, "1": 1, "2": 2, "log_run": run.bit_length() - 1, "log_tile": tile.bit_length() - 1, "log_tile+1": tile.bit_length()}[name]


def omega(log_n: int) -> int:
    return pow(M.FR_ROOT_OF_UNITY, 1 << (M.FR_S - log_n), R)


def points(log_n: int) -> list:
    """a fixed random value, 0, 2, r - 1, 1 = omega^0, omega, omega^(n/2) = -1, omega^(n-1), an element of order 2 n (not in the domain)"""
    n, w = 1 << log_n, omega(log_n)
    return [P.Z_FIXED, 0, 2, R - 1, 1, w, pow(w, n // 2, R), pow(w, n - 1, R), omega(log_n + 1)]


@functools.lru_cache(maxsize=None)
def evals_rows(log_n: int) -> np.ndarray:
    return inputs.random_fr_mont(1 << log_n, seed=4100 + log_n)


def evals_divide(lib, evals: np.ndarray, zs, q_stride=None, with_q=True):
    """-> (the whole (B, q_stride, 4) quotient buffer with its sentinels or None, (B, 4) values)"""
    import torch

    n, b = evals.shape[0], len(zs)
    q_stride = n if q_stride is None else q_stride
    q = torch.full((b, q_stride, 4), SENTINEL, dtype=torch.int64, device="cuda") if with_q else None
    values = torch.full((b, 4), SENTINEL, dtype=torch.int64, device="cuda")
    d_e, z = _dev(evals), np.concatenate([P.mont(v) for v in zs])
    rc = lib.mi355zk_bn254_fr_evals_divide_dev(C.c_void_p(q.data_ptr()) if with_q else None, q_stride, C.c_void_p(values.data_ptr()), C.c_void_p(d_e.data_ptr()),
                                               n.bit_length() - 1, z.ctypes.data_as(C.c_void_p), b, None)
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(_host(d_e), evals)
    return (_host(q) if with_q else None), _host(values)


_COEFFS = {}


def coefficient_route(zk, worker, log_n: int, zs):
    """(values as (B, 4) raw words, quotient evaluations as (B, n, 4)) through ifft, kzg.evaluate, kzg.divide and one fft per quotient"""
    import torch

    n = 1 << log_n
    if log_n not in _COEFFS:   # the ifft of the evaluations, once per size
        dom = zk.EvaluationDomain(_dev(evals_rows(log_n)), log_n)
        dom.ifft(worker)
        _COEFFS[log_n] = dom.into_coeffs()
    coeffs = _COEFFS[log_n]
    values = zk.kzg.evaluate(coeffs, zs)
    q, rems = zk.kzg.divide(coeffs, zs)
    assert rems == values
    padded = torch.zeros((len(zs), n, 4), dtype=torch.int64, device="cuda")
    padded[:, :n - 1] = q
    for j in range(len(zs)):
        dom = zk.EvaluationDomain(padded[j], log_n)
        dom.fft(worker)
    return P.rows([v * P.MONT % R for v in values]), _host(padded)


def big_int_model(log_n: int, z: int):
    """(the raw word of p(z), the raw words of the quotient's evaluations): interpolation, kate_divison and Horner in Python ints"""
    n, w = 1 << log_n, omega(log_n)
    f = P.ints(evals_rows(log_n))                       # raw words: the model is linear, so it runs on them as they are
    winv, ninv = pow(w, -1, R), pow(n, -1, R)
    c = [ninv * sum(f[i] * pow(winv, i * k, R) for i in range(n)) % R for k in range(n)]
    q, rem = P.kate_division(c, z)
    return rem, [P.horner(q, pow(w, i, R)) for i in range(n)]


def _check(lib, zk, worker, log_n, zs):
    q, values = evals_divide(lib, evals_rows(log_n), zs)
    want_values, want_q = coefficient_route(zk, worker, log_n, zs)
    assert np.array_equal(values, want_values), (log_n, [hex(z) for z in zs])
    assert np.array_equal(q, want_q), (log_n, [hex(z) for z in zs])
    if log_n <= 5:
        for j, z in enumerate(zs):
            rem, qe = big_int_model(log_n, z)
            assert np.array_equal(values[j], P.rows([rem])[0]) and np.array_equal(q[j], P.rows(qe)), (log_n, hex(z))


@pytest.mark.parametrize("b", [1, 3, 65])
@pytest.mark.parametrize("log_name", LOG_NAMES)
def test_values_and_quotients_match_the_coefficient_route(lib, zk, worker, log_name, b):
    log_n = log_n_of(log_name, lib)
    zs = points(log_n)
    if b == 65:
        groups = [(zs * 8)[:65]]
    else:
        groups = [zs[i:i + b] for i in range(0, len(zs), b)]
    for group in groups:
        _check(lib, zk, worker, log_n, group)


def test_python_layer_and_values_only(lib, zk, worker):
    log_n = log_n_of("log_tile", lib)
    zs = points(log_n)
    want_values, want_q = coefficient_route(zk, worker, log_n, zs)
    d = _dev(evals_rows(log_n))
    assert zk.kzg.evaluate_evals(d, zs) == zk.kzg.evaluate(_COEFFS[log_n], zs)
    q, values = zk.kzg.divide_evals(d, zs)
    assert q.shape == (len(zs), 1 << log_n, 4) and np.array_equal(_host(q), want_q) and values == zk.kzg.evaluate(_COEFFS[log_n], zs)
    none, only = evals_divide(lib, evals_rows(log_n), zs, with_q=False)     # d_q == NULL still writes the values
    assert none is None and np.array_equal(only, want_values)
    with pytest.raises(ValueError):
        zk.kzg.evaluate_evals(d[:3], zs)
    with pytest.raises(ValueError):
        zk.kzg.divide_evals(d, [])


def test_strided_quotients_leave_the_gaps_alone(lib, zk, worker):
    log_n = log_n_of("log_run", lib)
    n, zs = 1 << log_n, points(log_n)[3:8]
    want_values, want_q = coefficient_route(zk, worker, log_n, zs)
    q, values = evals_divide(lib, evals_rows(log_n), zs, q_stride=n + 3)
    assert np.array_equal(values, want_values) and np.array_equal(q[:, :n], want_q)
    assert (q[:, n:].view(np.int64) == SENTINEL).all()


def test_refusals(lib, zk):
    import torch

    bad = zk.lib.ERR_BAD_ARGS
    buf = torch.full((64, 4), SENTINEL, dtype=torch.int64, device="cuda")
    p = buf.data_ptr()
    ev, vals, q = C.c_void_p(p), C.c_void_p(p + 8 * 32), C.c_void_p(p + 16 * 32)
    z = np.concatenate([P.mont(3), P.mont(4)])
    zp = z.ctypes.data_as(C.c_void_p)
    f = lib.mi355zk_bn254_fr_evals_divide_dev
    assert f(q, 8, vals, None, 3, zp, 2, None) == bad
    assert f(q, 8, None, ev, 3, zp, 2, None) == bad
    assert f(q, 8, vals, ev, 3, None, 2, None) == bad
    assert f(q, 8, vals, ev, 29, zp, 2, None) == bad
    assert f(q, 8, vals, ev, 3, zp, 0, None) == bad
    assert f(q, 8, vals, ev, 3, zp, zk.lib.POLY_MAX_POINTS + 1, None) == bad
    assert f(q, 7, vals, ev, 3, zp, 2, None) == bad                                 # q_stride < n
    assert f(C.c_void_p(p + 7 * 32), 8, C.c_void_p(p + 40 * 32), ev, 3, zp, 1, None) == bad   # the quotient starts in the evaluations' last element
    assert f(C.c_void_p(p + 9 * 32), 8, vals, ev, 3, zp, 2, None) == bad            # ... in values[1]
    torch.cuda.synchronize()
    assert (_host(buf).view(np.int64) == SENTINEL).all()
