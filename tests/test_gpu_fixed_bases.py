"""Linear combinations over a set of fixed G1 bases on the device (csrc/fixed_base.hip: fixed_bases_lincomb_kernel, fixed_bases_join_kernel)
against the oracle, byte for byte: planned and forced slices, the rows whose partial sums meet the exceptional cases of the group law in
the first, a middle and the last lane, the chunk boundary against the single-base table, two streams, and the empty call."""
import ctypes as C
import threading

import numpy as np
import pytest

import fixed_base_cases as FB
import fixed_bases_cases as FBS
import inputs

pytestmark = pytest.mark.gpu

R = FBS.R
SHAPES = ((1, 1), (1, 40), (3, 7), (257, 3), (64, 0))


def _dev(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _rows(n, logs, seed):
    """n rows over the bases: uniform scalars, with the exceptional rows (as many as fit) in the first, a middle and the last lane"""
    n_bases = len(logs)
    if n_bases == 0:
        return np.zeros((n, 0, 4), np.uint64)
    scalars = inputs.random_scalars(n * n_bases, seed=seed).reshape(n, n_bases, 4).copy()
    special = FBS.scalar_rows([row for _, row in FBS.exceptional_rows(logs)])
    edge = FB.limbs(FB.edge_scalars())
    special = np.concatenate([special, edge[:n_bases * (len(edge) // n_bases)].reshape(-1, n_bases, 4)[:3]]) if n_bases <= len(edge) else special
    places = [0, n - 1, n // 2] + [i for i in range(1, n - 1) if i != n // 2]
    for k, row in enumerate(special[:n]):
        scalars[places[k]] = row
    return np.ascontiguousarray(scalars)


@pytest.fixture(scope="module")
def cases():
    """per shape: bases, first, scalars and the oracle's records for first absent and first a point -- computed once"""
    first = FBS.points([FBS.FIRST_LOG])[0]
    out = {}
    for n, n_bases in SHAPES:
        logs = FBS.base_logs(n_bases, seed=9400 + n_bases)
        bases = FBS.points(logs)
        scalars = _rows(n, logs, seed=9450 + n)
        out[(n, n_bases)] = {"bases": bases, "first": first, "scalars": scalars, "want_none": FBS.want_lincomb(bases, None, scalars),
                             "want_first": FBS.want_lincomb(bases, first, scalars)}
    return out


@pytest.mark.parametrize("n,n_bases", SHAPES)
def test_lincomb_matches_the_oracle(zk, worker, cases, n, n_bases):
    c = cases[(n, n_bases)]
    tab = zk.pairing.FixedBasesTable(c["bases"])
    d_k, d_first = _dev(c["scalars"]), _dev(c["first"])
    for slice_len in sorted({0, 1, 3, max(n_bases, 1)}):
        got = _host(tab.lincomb(d_k, None, slice_len))
        assert got.shape == (n, 8) and np.array_equal(got, c["want_none"]), (slice_len, np.nonzero((got != c["want_none"]).any(axis=1))[0][:8])
        got = _host(tab.lincomb(d_k, d_first, slice_len))
        assert np.array_equal(got, c["want_first"]), (slice_len, "first", np.nonzero((got != c["want_first"]).any(axis=1))[0][:8])
        zero_first = _host(tab.lincomb(d_k, _dev(np.zeros(8, np.uint64)), slice_len))          # the identity record as `first`
        assert np.array_equal(zero_first, c["want_none"]), (slice_len, "identity first")
    if n_bases == 0:
        assert np.array_equal(c["want_first"], np.tile(c["first"], (n, 1)))                     # `first` n times


def test_exceptional_rows_on_the_device(zk, worker, cases):
    """the group law's answers stated directly for the rows planted in lanes 0 and n - 1 of the (257, 3) case, under every slicing"""
    c = cases[(257, 3)]
    named = [name for name, _ in FBS.exceptional_rows(FBS.base_logs(3, seed=9403))]
    assert named[:2] == ["cancel", "double"]
    tab = zk.pairing.FixedBasesTable(c["bases"])
    ten_p = FBS.want_lincomb(c["bases"][:1], None, FBS.scalar_rows([[10]]))[0]
    for slice_len in (0, 1, 3):
        got = _host(tab.lincomb(_dev(c["scalars"]), _dev(c["first"]), slice_len))
        assert np.array_equal(got[0], c["first"]), slice_len                                     # k P + (r - k) P + first
        none = _host(tab.lincomb(_dev(c["scalars"]), None, slice_len))
        assert not none[0].any() and np.array_equal(none[256], ten_p), slice_len                # the identity; 5 P + 5 P
    where = [i for i in range(257) if not c["want_first"][i].any()]
    assert where, "the row whose sum is -first is in the batch"


def test_chunk_boundary_against_the_single_base_table(zk, worker):
    """n = 2^18 + 3 rows over one base without `first` is FixedBaseTable.mul of the same scalars: the second launch starts where it must"""
    import torch

    n = (1 << 18) + 3
    base = FBS.points([0x1234567 % R])[0]
    d_k = _dev(inputs.random_scalars(n, seed=9460))
    want = zk.FixedBaseTable(base).mul(d_k)
    got = zk.pairing.FixedBasesTable(base.reshape(1, 8)).lincomb(d_k.reshape(n, 1, 4))
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    # and with two lanes a row across that boundary: two equal bases, half the rows in the second launch
    n2 = (1 << 17) + 1
    tab2 = zk.pairing.FixedBasesTable(np.stack([base, base]))
    d_k2 = d_k[:2 * n2].reshape(n2, 2, 4).contiguous()
    one, two = tab2.lincomb(d_k2, None, 2), tab2.lincomb(d_k2, None, 1)
    torch.cuda.synchronize()
    assert torch.equal(one, two)


def test_two_streams_agree(zk, worker, cases):
    import torch

    c = cases[(257, 3)]
    tab = zk.pairing.FixedBasesTable(c["bases"])
    d_k, d_first = _dev(c["scalars"]), _dev(c["first"])
    torch.cuda.synchronize()
    results = [None, None]

    def call(k):
        with torch.cuda.stream(torch.cuda.Stream()):
            r = tab.lincomb(d_k, d_first, k)              # one slice on one stream, three on the other
            torch.cuda.current_stream().synchronize()
            results[k] = _host(r)

    threads = [threading.Thread(target=call, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert np.array_equal(results[0], c["want_first"]) and np.array_equal(results[1], c["want_first"])


def test_empty_call_and_refusals(zk, worker, cases):
    import torch

    c = cases[(3, 7)]
    tab = zk.pairing.FixedBasesTable(c["bases"])
    assert tuple(tab.lincomb(torch.empty((0, 7, 4), dtype=torch.int64, device="cuda")).shape) == (0, 8)
    lib = zk.lib.load()
    out = torch.zeros((3, 8), dtype=torch.int64, device="cuda")
    d_k = _dev(c["scalars"])
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    comb = lib.mi355zk_bn254_g1_fixed_bases_lincomb_dev
    assert comb(None, p(tab.table), 7, None, p(d_k), 3, 0, None) == 3
    assert comb(p(out), None, 7, None, p(d_k), 3, 0, None) == 3
    assert comb(p(out), p(tab.table), 7, None, None, 3, 0, None) == 3
    assert comb(p(out), p(tab.table), 7, None, p(d_k), 1 << 31, 0, None) == 3
    torch.cuda.synchronize()
    assert not out.any()                                     # nothing was launched
    off = inputs.G1_GEN_RAW.copy()
    off[4] ^= 1
    with pytest.raises(ValueError):
        zk.pairing.FixedBasesTable(np.stack([inputs.G1_GEN_RAW, off]))
