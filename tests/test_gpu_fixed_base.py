"""Fixed-base window tables on the device (csrc/fixed_base.hip) and mi355zk_bn254_fr_powers_dev, against the oracle and Python big ints."""
import ctypes as C

import numpy as np
import pytest

import bn254_model as M
import fixed_base_cases as FB
import inputs
import oracle_lib as O

pytestmark = pytest.mark.gpu

R = M.R_ORDER
SIZES = (1, 63, 64, 65, 257, 4099)
N_MAX = max(SIZES)


def _dev(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.fixture(scope="module")
def scalars():
    """4099 canonical scalars: the recoding's edge list, then uniform ones"""
    edge = FB.limbs(FB.edge_scalars())
    return np.ascontiguousarray(np.concatenate([edge, inputs.random_scalars(N_MAX - edge.shape[0], seed=9200)]))


@pytest.fixture(scope="module")
def bases():
    """per group: the generator and (G1) a random multiple of it"""
    other = O.G1.mul_many_affine(inputs.G1_GEN_RAW, inputs.random_scalars(1, seed=9201))[0]
    return {1: [inputs.G1_GEN_RAW, np.ascontiguousarray(other)], 2: [inputs.G2_GEN_RAW]}


_want_cache = {}


def _want(group, which, base, scalars):
    """the oracle's k[i] * base, computed once per base and shared"""
    if (group, which) not in _want_cache:
        _want_cache[(group, which)] = (O.G1 if group == 1 else O.G2).mul_many_affine(base, scalars)
    return _want_cache[(group, which)]


@pytest.mark.parametrize("group,which", [(1, 0), (1, 1), (2, 0)])
def test_table_mul_matches_the_oracle(zk, worker, scalars, bases, group, which):
    base = bases[group][which]
    want = _want(group, which, base, scalars)
    tab = zk.FixedBaseTable(base)
    mont = np.array([M.to_limbs(M.to_mont(k, R)) for k in FB.ints(scalars)], dtype=np.uint64)
    d_k, d_m = _dev(scalars), _dev(mont)
    for n in SIZES:
        got = _host(tab.mul(d_k[:n].contiguous()))
        assert got.shape == want[:n].shape and np.array_equal(got, want[:n]), (group, n, np.nonzero((got != want[:n]).any(axis=1))[0][:8])
        got = _host(tab.mul(d_m[:n].contiguous(), montgomery=True))
        assert np.array_equal(got, want[:n]), (group, n, "montgomery")
    assert tab.mul(d_k[:0].contiguous()).shape[0] == 0
    fn = zk.lib.load().mi355zk_bn254_g1_fixed_base_mul_dev if group == 1 else zk.lib.load().mi355zk_bn254_g2_fixed_base_mul_dev
    assert fn(None, None, None, 0, 0, None) == 0                # n == 0: nothing to do, nothing to look at


@pytest.mark.parametrize("group", [1, 2])
def test_table_mul_agrees_with_batch_mul(zk, worker, scalars, bases, group):
    import torch

    base = np.ascontiguousarray(bases[group][0])
    d_k = _dev(scalars)
    old = torch.empty((N_MAX, 8 * group), dtype=torch.int64, device="cuda")
    fn = zk.lib.load().mi355zk_bn254_g1_batch_mul_dev if group == 1 else zk.lib.load().mi355zk_bn254_g2_batch_mul_dev
    assert fn(C.c_void_p(old.data_ptr()), base.ctypes.data_as(C.c_void_p), C.c_void_p(d_k.data_ptr()), N_MAX, None) == 0
    new = zk.FixedBaseTable(base).mul(d_k)
    torch.cuda.synchronize()
    assert torch.equal(old, new)


def test_refusals(zk, worker, scalars):
    import torch
    from test_g2_subgroup import _twist_point

    lib = zk.lib.load()
    b1, b2 = lib.mi355zk_fixed_base_table_bytes(1), lib.mi355zk_fixed_base_table_bytes(2)
    t = torch.zeros(b2 // 8, dtype=torch.int64, device="cuda")
    p = lambda a: np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)  # noqa: E731
    build1, build2 = lib.mi355zk_bn254_g1_fixed_base_build_dev, lib.mi355zk_bn254_g2_fixed_base_build_dev
    assert build1(C.c_void_p(t.data_ptr()), b1, p(np.zeros(8, np.uint64)), None) == 3            # the identity
    assert build2(C.c_void_p(t.data_ptr()), b2, p(np.zeros(16, np.uint64)), None) == 3
    off = inputs.G1_GEN_RAW.copy()
    off[4:] = O.fe_add(0, off[4:], off[4:])                                                       # (x, 2 y): on no curve
    assert build1(C.c_void_p(t.data_ptr()), b1, p(off), None) == 3
    assert build2(C.c_void_p(t.data_ptr()), b2, p(_twist_point(77)), None) == 3                   # on the twist, outside the subgroup
    assert build1(C.c_void_p(t.data_ptr()), b1 - 1, p(inputs.G1_GEN_RAW), None) == 3              # a short table
    assert build2(C.c_void_p(t.data_ptr()), b1, p(inputs.G2_GEN_RAW), None) == 3
    assert build1(None, b1, p(inputs.G1_GEN_RAW), None) == 3
    with pytest.raises(ValueError):
        zk.FixedBaseTable(np.zeros(8, np.uint64))
    assert not t.any()                                                                            # refused before any device work
    tab = zk.FixedBaseTable(inputs.G1_GEN_RAW)
    d_k = _dev(scalars[:4])
    out = torch.zeros((4, 8), dtype=torch.int64, device="cuda")
    mul = lib.mi355zk_bn254_g1_fixed_base_mul_dev
    assert mul(C.c_void_p(out.data_ptr()), C.c_void_p(tab.table.data_ptr()), C.c_void_p(d_k.data_ptr()), 4, 2, None) == 3   # unknown flag
    assert mul(None, C.c_void_p(tab.table.data_ptr()), C.c_void_p(d_k.data_ptr()), 4, 0, None) == 3
    assert mul(C.c_void_p(out.data_ptr()), C.c_void_p(tab.table.data_ptr()), C.c_void_p(d_k.data_ptr()), 1 << 31, 0, None) == 3
    torch.cuda.synchronize()
    assert not out.any()


@pytest.mark.parametrize("group", [1, 2])
def test_out_of_range_scalars_leave_the_others_exact(zk, worker, scalars, bases, group):
    base = bases[group][0]
    ks = scalars[:66].copy()
    ks[7] = FB.limbs([(1 << 256) - 1])[0]
    ks[40] = FB.limbs([R])[0]
    want = _want(group, 0, base, scalars)[:66]
    got = _host(zk.FixedBaseTable(base).mul(_dev(ks)))
    keep = np.ones(66, bool)
    keep[[7, 40]] = False
    assert np.array_equal(got[keep], want[keep])


@pytest.mark.parametrize("n", [1, 15, 16, 17, 4099])
def test_fr_powers(zk, worker, n):
    import torch

    lib = zk.lib.load()
    rnd = FB.ints(inputs.random_scalars(3, seed=9210))
    out = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    for base in (0, 1, R - 1, rnd[0]):
        for coeff in (1, rnd[1]):
            b = np.array(M.to_limbs(M.to_mont(base, R)), dtype=np.uint64)
            c = np.array(M.to_limbs(M.to_mont(coeff, R)), dtype=np.uint64)
            assert lib.mi355zk_bn254_fr_powers_dev(C.c_void_p(out.data_ptr()), b.ctypes.data_as(C.c_void_p), c.ctypes.data_as(C.c_void_p), n, None) == 0
            got = [M.from_mont(v, R) for v in FB.ints(_host(out))]
            want, cur = [], coeff
            for _ in range(n):
                want.append(cur)
                cur = cur * base % R
            assert got == want, (n, hex(base), hex(coeff))
    one = np.array(M.to_limbs(M.to_mont(1, R)), dtype=np.uint64)
    assert lib.mi355zk_bn254_fr_powers_dev(None, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), 0, None) == 0
    assert lib.mi355zk_bn254_fr_powers_dev(None, one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), 4, None) == 3
    assert lib.mi355zk_bn254_fr_powers_dev(C.c_void_p(out.data_ptr()), None, one.ctypes.data_as(C.c_void_p), 1, None) == 3
    assert lib.mi355zk_bn254_fr_powers_dev(C.c_void_p(out.data_ptr()), one.ctypes.data_as(C.c_void_p), one.ctypes.data_as(C.c_void_p), 1 << 32, None) == 3
