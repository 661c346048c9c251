"""The random exponents of merge_pairs generated on the device (csrc/fr_random.hip): the kernel against the host run of the same generator
(which tests/test_fr_random_host.py holds against an independent ChaCha20), and merge_pairs over generated exponents against merge_pairs
fed the same exponents by the caller."""
import numpy as np
import pytest

import inputs
import oracle_lib as O

pytestmark = pytest.mark.gpu

KEY = bytes(range(100, 132))
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


@pytest.fixture(scope="module")
def points():
    """one progression per group, shared by the tests below and never written"""
    return {1: inputs.bases_progression_cpu(1, 4098, seed=5101), 2: inputs.bases_progression_cpu(2, 1026, seed=5102)}


@pytest.mark.parametrize("first", [0, 1, (1 << 32) - 1, (1 << 33) + 2], ids=("even0", "odd1", "odd_carry", "even_high"))
def test_fr_random_dev_equals_the_host_run(zk, worker, first):
    """n around the block (two scalars), the wave (64 lanes = 128 scalars) and the 256-lane workgroup; even and odd `first`: half-blocks at
    both ends.  The rows before and after the range keep their sentinel."""
    import torch

    for n in (1, 2, 3, 63, 64, 65, 1025):
        buf = torch.full((n + 2, 4), SENTINEL, dtype=torch.int64, device="cuda")
        out = buf[1:n + 1]
        rc = zk.lib.load().mi355zk_bn254_fr_random_dev(out.data_ptr(), n, zk.ceremony._chacha_key(KEY), 9, first, None)
        assert rc == 0
        torch.cuda.synchronize()
        got = buf.cpu().numpy().view(np.uint64)
        assert (got[0] == SENTINEL).all() and (got[-1] == SENTINEL).all(), (n, "wrote outside the range")
        assert np.array_equal(got[1:-1], zk.ceremony.fr_random_host(n, KEY, 9, first)), n
    assert np.array_equal(zk.ceremony.fr_random(65, KEY, 9, first).cpu().numpy().view(np.uint64), zk.ceremony.fr_random_host(65, KEY, 9, first))


def test_fr_random_dev_argument_rules(zk, worker):
    import torch

    lib = zk.lib.load()
    buf = torch.full((4, 4), SENTINEL, dtype=torch.int64, device="cuda")
    key = zk.ceremony._chacha_key(KEY)
    assert lib.mi355zk_bn254_fr_random_dev(buf.data_ptr(), 0, key, 0, 0, None) == 0          # launches nothing
    assert lib.mi355zk_bn254_fr_random_dev(buf.data_ptr() + 8, 1, key, 0, 0, None) == zk.lib.ERR_BAD_ARGS   # 16-byte alignment
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    assert zk.ceremony.fr_random(0, KEY).shape == (0, 4)


@pytest.mark.parametrize("group,n", [(1, 1), (1, 2), (1, 100), (1, 4097), (2, 1), (2, 100), (2, 1025)])
def test_merge_pairs_random_dev_equals_merge_pairs_with_the_same_scalars(zk, worker, points, group, n):
    G = O.G1 if group == 1 else O.G2
    v = _dev(points[group][:n + 1])
    v1, v2 = v[:n], v[1:]
    rho = _dev(zk.ceremony.fr_random_host(n, KEY, 3))
    want_s, want_sx = zk.ceremony.merge_pairs(v1, v2, rho)
    got_s, got_sx = zk.ceremony.merge_pairs_random(v1, v2, KEY, 3)
    assert G.to_affine(got_s).tobytes() == G.to_affine(want_s).tobytes()
    assert G.to_affine(got_sx).tobytes() == G.to_affine(want_sx).tobytes()
    assert G.to_affine(got_s).any()
    other_s, _ = zk.ceremony.merge_pairs_random(v1, v2, KEY, 4)              # another stream id: other exponents
    assert G.to_affine(other_s).tobytes() != G.to_affine(got_s).tobytes()
    ps, psx = zk.ceremony.power_pairs_random(v, KEY, 3)
    assert G.to_affine(ps).tobytes() == G.to_affine(want_s).tobytes() and G.to_affine(psx).tobytes() == G.to_affine(want_sx).tobytes()


@pytest.mark.parametrize("group", [1, 2])
def test_host_merge_pairs_random_is_the_same_point_for_every_piece_size(zk, worker, points, group, monkeypatch):
    """n = 100, v2 = v1 + one record (power_pairs): pieces of 16 and of 48 points -- each fills its exponents from the piece's first index --
    give the sums of the one-piece call and of the device-resident call."""
    G = O.G1 if group == 1 else O.G2
    n = 100
    v = np.ascontiguousarray(points[group][:n + 1])
    monkeypatch.delenv("MI355ZK_DENSE_PIECE_TEST", raising=False)
    one_s, one_sx = (G.to_affine(p) for p in zk.ceremony.merge_pairs_random_host(v[:n], v[1:], KEY, 7))
    dv = _dev(v)
    dev_s, dev_sx = (G.to_affine(p) for p in zk.ceremony.merge_pairs_random(dv[:n], dv[1:], KEY, 7))
    assert one_s.tobytes() == dev_s.tobytes() and one_sx.tobytes() == dev_sx.tobytes()
    for piece in ("16", "48"):
        monkeypatch.setenv("MI355ZK_DENSE_PIECE_TEST", piece)
        s, sx = (G.to_affine(p) for p in zk.ceremony.merge_pairs_random_host(v[:n], v[1:], KEY, 7))
        assert s.tobytes() == one_s.tobytes() and sx.tobytes() == one_sx.tobytes(), piece
        # and the host form with the caller's exponents, same pieces: the stream is what the caller would have uploaded
        hs, hsx = (G.to_affine(p) for p in zk.ceremony.merge_pairs_host(v[:n], v[1:], zk.ceremony.fr_random_host(n, KEY, 7)))
        assert hs.tobytes() == one_s.tobytes() and hsx.tobytes() == one_sx.tobytes(), piece
