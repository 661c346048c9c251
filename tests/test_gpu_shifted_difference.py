"""mi355zk_bn254_g1_shifted_difference_dev (csrc/point_diff.hip) on the device: the cases of tests/test_shifted_difference_host.py byte for
byte against the host run of the same lane routine and against the integers, a launch of more than one block with a ragged last group,
the empty call, and the sparse-product route of ceremony.prepare_phase2 on the same vector."""
import ctypes as C

import numpy as np
import pytest

import prepare_phase2_cases as P

pytestmark = pytest.mark.gpu


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()


def _np(t) -> np.ndarray:
    return t.cpu().numpy().view(np.uint64)


def _host(zk, points: np.ndarray, shift: int, n_out: int) -> np.ndarray:
    out = np.zeros((n_out, 8), dtype=np.uint64)
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    assert zk.lib.load().mi355zk_selftest_g1_shifted_difference(p(out), p(points), points.shape[0], shift, n_out) == 0
    return out


@pytest.mark.parametrize("case", P.CASES, ids=P.CASE_IDS)
def test_device_matches_the_host_twin_and_the_integers(zk, worker, case):
    _, multiples, shift, n_out = case
    points = P.raw(multiples)
    got = _np(zk.ceremony.shifted_difference(_dev(points), shift, n_out))
    assert np.array_equal(got, _host(zk, points, shift, n_out))
    assert np.array_equal(got, P.expected(multiples, shift, n_out))


def test_more_than_one_block_with_a_ragged_last_group(zk, worker):
    """256 * K outputs fill one block: one block and 37 outputs more, two full groups and a group of five in the second block"""
    import torch

    n_out, shift = 256 * P.K + 37, 5
    assert n_out % (256 * P.K) and n_out > 256 * P.K and n_out % P.K
    multiples = P.mixed(n_out + shift, seed=99)
    points = P.raw(multiples)
    d_points = _dev(points)
    out = torch.full((n_out + 1, 8), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    got = zk.ceremony.shifted_difference(d_points, shift, n_out, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert np.array_equal(_np(got), P.expected(multiples, shift, n_out))
    assert np.array_equal(_np(got), _host(zk, points, shift, n_out))
    assert bool((out[n_out] == 0x5A5A5A5A5A5A5A5A).all())             # nothing is written past n_out
    assert np.array_equal(_np(d_points), points)                      # the input is read only


def test_no_output_is_a_no_op(zk, worker):
    points = _dev(P.raw([1, 2, 3]))
    assert zk.ceremony.shifted_difference(points, 3, 0).shape == (0, 8)
    assert zk.lib.load().mi355zk_bn254_g1_shifted_difference_dev(None, None, 3, 2, 0, None) == 0
    for shift, n_out in ((0, 1), (2, 2), (4, 0)):
        with pytest.raises(ValueError):
            zk.ceremony.shifted_difference(points, shift, n_out)


def test_h_bases_are_those_of_the_sparse_product(zk, worker):
    """the two-term rows of ceremony.prepare_phase2 -- the independent path -- give the same bytes for generic points"""
    m = 16
    multiples = [(3 * i * i + 5 * i + 1) % 47 + 1 for i in range(2 * m - 1)]   # no infinity, no equal or opposite neighbours m apart
    assert all(multiples[i + m] != multiples[i] for i in range(m - 1))
    tau_g1 = _dev(P.raw(multiples))
    acc = {"tau_g1": tau_g1, "tau_g2": _dev(np.tile(np.array(zk.ceremony.G2_ONE_RAW, dtype=np.uint64), (m, 1))), "alpha_g1": tau_g1[:m], "beta_g1": tau_g1[:m],
           "beta_g2": _dev(np.array(zk.ceremony.G2_ONE_RAW, dtype=np.uint64).reshape(1, 16))}
    want = _np(zk.ceremony.prepare_phase2(acc, m)["h"])
    assert np.array_equal(_np(zk.ceremony.shifted_difference(tau_g1, m, m - 1)), want)
    assert np.array_equal(want, P.expected(multiples, m, m - 1))
