"""The Python layer over the scans (phase2-bn254_amd/grand_product.py): grand_product_polynomials against a serial restatement of
GrandProductArgument::new (sonic/unhelped/grand_product_argument.rs:119-163) in Python big ints, its results under kzg.commit_many, and
permutation_product for a true and a false statement, both first settled in big ints on the CPU."""
import ctypes as C
import random

import numpy as np
import pytest

import fixed_base_cases as FB
import fr_scan_cases as V
import inputs
import oracle_lib as O

pytestmark = pytest.mark.gpu
R, MONT = V.R, V.MONT
TAU = 0x2F0E1D2C3B4A59687796A5B4C3D2E1F00F1E2D3C4B5A69788796A5B4C3D2E1F % R
BETA = 0x1B7E4D3C2A190807F6E5D4C3B2A1908F7E6D5C4B3A29180706F5E4D3C2B1A09 % R
GAMMA = 0x2468ACE013579BDF02468ACE13579BDF2468ACE013579BDF02468ACE13579BD % R
ONE = V.rows([MONT])[0]


@pytest.fixture(scope="module")
def lib(zk, worker):
    return zk.lib.load()


def _dev(a: np.ndarray):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def _host(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def _mont(vals) -> np.ndarray:
    """field elements as ints -> (len, 4) Montgomery rows"""
    return V.rows([v % R * MONT % R for v in vals])


def _serial_grand_product(a, b):
    """grand_product_argument.rs:119-163 for one pair, on field elements as ints: c_coeff starts at one and is multiplied by every a in turn,
    each value pushed; a_poly is a, then ZERO where v would stand; c gets a one; a fresh c_coeff runs over b; v is the inverse of a's product."""
    c_poly, a_poly, c = [], [], 1
    for x in a:
        c = c * x % R
        c_poly.append(c)
    a_poly.extend(a)
    v = pow(c, -1, R)
    a_poly.append(0)
    c = 1
    c_poly.append(c)
    for x in b:
        c = c * x % R
        c_poly.append(c)
    a_poly.extend(b)
    return a_poly, c_poly, v


@pytest.fixture(scope="module")
def pairs(lib):
    """three pairs of n = tile + 1 non-zero elements, each b a shuffle of its a"""
    n = V.geometry(lib)[1] + 1
    rnd = random.Random(4242)
    out = []
    for _ in range(3):
        a = [rnd.randrange(1, R) for _ in range(n)]
        b = a[:]
        rnd.shuffle(b)
        out.append((a, b))
    return out


def test_grand_product_polynomials_match_the_serial_reference(lib, zk, pairs):
    import torch

    n = len(pairs[0][0])
    a_polys, c_polys, v = zk.grand_product.grand_product_polynomials([(_dev(_mont(a)), _dev(_mont(b))) for a, b in pairs])
    assert a_polys.shape == c_polys.shape == (3, 2 * n + 1, 4) and v.shape == (3, 4)
    got_a, got_c, got_v = _host(a_polys), _host(c_polys), _host(v)
    for p, (a, b) in enumerate(pairs):
        want_a, want_c, want_v = _serial_grand_product(a, b)
        assert np.array_equal(got_a[p], _mont(want_a)), p
        assert np.array_equal(got_c[p], _mont(want_c)), p
        assert np.array_equal(got_v[p], _mont([want_v])[0]), p
        assert (got_c[p, n] == ONE).all() and np.array_equal(got_c[p, n - 1], got_c[p, 2 * n])
    check = v.clone()                                   # v c[n-1] == 1, through mul_assign_dev
    last = c_polys[:, n - 1].contiguous()
    assert lib.mi355zk_bn254_fr_mul_assign_dev(C.c_void_p(check.data_ptr()), C.c_void_p(last.data_ptr()), 3, None) == 0
    torch.cuda.synchronize()
    assert (_host(check) == ONE).all()


def test_a_pair_that_is_no_shuffle_is_refused(lib, zk, pairs):
    devs = [(_dev(_mont(a)), _dev(_mont(b))) for a, b in pairs]
    b = list(pairs[1][1])
    b[3] = (b[3] + 1) % R or 1
    devs[1] = (devs[1][0], _dev(_mont(b)))
    with pytest.raises(ValueError, match="pair 1"):
        zk.grand_product.grand_product_polynomials(devs)
    with pytest.raises(ValueError):
        zk.grand_product.grand_product_polynomials([])
    with pytest.raises(ValueError):
        zk.grand_product.grand_product_polynomials([(devs[0][0], devs[0][1][:-1])])


def test_commit_many_takes_the_polynomials_as_they_are(lib, zk, pairs):
    n = len(pairs[0][0])
    powers, cur = [], 1
    for _ in range(2 * n + 1):
        powers.append(cur)
        cur = cur * TAU % R
    g1 = O.G1.mul_many_affine(inputs.G1_GEN_RAW, FB.limbs(powers))
    g2 = O.G2.mul_many_affine(inputs.G2_GEN_RAW, FB.limbs([1, TAU]))
    srs = zk.kzg.srs_from_points(_dev(g1), _dev(g2[0]), _dev(g2[1]))
    _, c_polys, _ = zk.grand_product.grand_product_polynomials([(_dev(_mont(a)), _dev(_mont(b))) for a, b in pairs])
    many = zk.kzg.commit_many(srs, c_polys)
    assert many.shape == (3, 8)
    for p in range(3):
        assert np.array_equal(many[p], zk.kzg.commit(srs, c_polys[p])), p


def _permutation_case(lib):
    """k = 3 columns of n = 2 run + 1 rows over six distinct values; the permutation rotates the cells of every class of equal values by one"""
    k, n = 3, 2 * V.geometry(lib)[0] + 1
    rnd = random.Random(777)
    pool = [rnd.randrange(1, R) for _ in range(6)]
    values = [[pool[rnd.randrange(6)] for _ in range(n)] for _ in range(k)]
    positions = [[j * n + i + 1 for i in range(n)] for j in range(k)]
    permuted = [[0] * n for _ in range(k)]
    for val in pool:
        cells = [(j, i) for j in range(k) for i in range(n) if values[j][i] == val]
        for (j, i), (j2, i2) in zip(cells, cells[1:] + cells[:1]):
            permuted[j][i] = positions[j2][i2]
    return values, positions, permuted


def _chain(values, positions, permuted, beta, gamma):
    """(Z[0 .. n), Z[n]) in big ints"""
    k, n = len(values), len(values[0])
    z, acc = [], 1
    for i in range(n):
        z.append(acc)
        num = den = 1
        for j in range(k):
            num = num * (values[j][i] + beta * positions[j][i] + gamma) % R
            den = den * (values[j][i] + beta * permuted[j][i] + gamma) % R
        acc = acc * num * pow(den, -1, R) % R
    return z, acc


def _cols(cols):
    return _dev(np.stack([_mont(c) for c in cols]))


def test_permutation_product_true_and_false_statements(lib, zk):
    values, positions, permuted = _permutation_case(lib)
    n = len(values[0])
    want_z, want_total = _chain(values, positions, permuted, BETA, GAMMA)
    assert want_total == 1 and any(v != 1 for v in want_z)              # settled on the CPU first: the statement is true, the chain not trivial
    z, total = zk.grand_product.permutation_product(_cols(values), _cols(positions), _cols(permuted), BETA, GAMMA)
    assert z.shape == (n, 4) and total.shape == (4,)
    assert np.array_equal(_host(z), _mont(want_z)) and (_host(total) == ONE).all()
    # one value changed inside a class of at least two cells: the multisets differ
    assert sum(row.count(values[0][0]) for row in values) >= 2
    wrong = [row[:] for row in values]
    wrong[0][0] = (wrong[0][0] + 1) % R
    bad_z, bad_total = _chain(wrong, positions, permuted, BETA, GAMMA)
    assert bad_total != 1                                                # ... and for THESE challenges the total shows it
    z, total = zk.grand_product.permutation_product(_cols(wrong), _cols(positions), _cols(permuted), BETA, GAMMA)
    assert np.array_equal(_host(z), _mont(bad_z)) and np.array_equal(_host(total), _mont([bad_total])[0])
    assert not (_host(total) == ONE).all()


def test_permutation_product_refuses_a_cancelled_denominator(lib, zk):
    values, positions, permuted = _permutation_case(lib)
    gamma = -(values[1][4] + BETA * permuted[1][4]) % R                 # the factor of column 1 in row 4 of the denominator is zero
    with pytest.raises(ZeroDivisionError, match="1 zero denominator"):
        zk.grand_product.permutation_product(_cols(values), _cols(positions), _cols(permuted), BETA, gamma)
    with pytest.raises(ValueError):
        zk.grand_product.permutation_product(_cols(values), _cols(positions), _cols(permuted)[:2], BETA, GAMMA)
