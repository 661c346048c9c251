"""xyzzu_from_affine_pair (csrc/curveu.hpp: how a G1 bucket opens) on the DEVICE, one pair per lane through mi355zk_selftest_dev_op
(MI355ZK_DEVOP_G1_ADD_AFFINE_PAIR), against tests/bn254_model.py big integers: random pairs under all four sign combinations, points whose
x or y is 0, 1, p - 1 (or the nearest coordinate the curve has), P, P under ++ / -- (doubling), P, P under +- and P, -P under ++
(infinity).  The affine normalisation of the returned accumulator is the model's sum exactly; its limbs are N-form and below X < 6p, Y,
ZZ, ZZZ < 2p; infinity is literal-zero ZZ; the record is xyzzu_to_r of that accumulator.  The ZK_CHAIN_MAD build (what msm_g1.hip ships)
returns the same words.  The same cases run on the host build under sanitizers in tests/test_pair_start_host.py."""
import numpy as np
import pytest

import field_edge_vectors as V
import pair_start_vectors as PV

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(zk, worker):
    return zk.lib.load()


def run(lib, rows, chain):
    inp = np.ascontiguousarray(np.array([inw for _, inw, _ in rows], dtype=np.uint32).reshape(len(rows), PV.IN_WORDS))
    out = np.zeros((len(rows), PV.OUT_WORDS), np.uint32)
    rc = lib.mi355zk_selftest_dev_op(PV.CODE | (V.CHAIN if chain else 0), 0, inp.ctypes.data, PV.IN_WORDS, out.ctypes.data, PV.OUT_WORDS, len(rows))
    assert rc == 0, "mi355zk_selftest_dev_op(G1_ADD_AFFINE_PAIR%s) returned %d" % ("|CHAIN" if chain else "", rc)
    return out


def test_pair_start_against_the_model(lib):
    rows = PV.cases()
    plain = run(lib, rows, False)
    bad = []
    for (name, _, want), outw in zip(rows, plain):
        try:
            PV.verify(name, outw, want)
        except AssertionError as e:
            bad.append(str(e))
    assert not bad, "%d of %d cases wrong, first:\n%s" % (len(bad), len(rows), "\n".join(bad[:5]))
    chain = run(lib, rows, True)
    diff = np.nonzero((plain != chain).any(axis=1))[0]
    assert diff.size == 0, "the plain and the ZK_CHAIN_MAD build differ in %d cases, first: %s" % (diff.size, rows[diff[0]][0])


def test_the_hook_refuses_other_shapes(lib):
    a, out = np.zeros(PV.IN_WORDS + 1, np.uint32), np.zeros(PV.OUT_WORDS + 1, np.uint32)
    f = lib.mi355zk_selftest_dev_op
    assert f(PV.CODE, 0, a.ctypes.data, PV.IN_WORDS + 1, out.ctypes.data, PV.OUT_WORDS, 1) != 0
    assert f(PV.CODE, 0, a.ctypes.data, PV.IN_WORDS, out.ctypes.data, PV.OUT_WORDS + 1, 1) != 0
    assert f(PV.CODE, 1, a.ctypes.data, PV.IN_WORDS, out.ctypes.data, PV.OUT_WORDS, 1) != 0      # no Fr form
    assert f(PV.CODE + 1, 0, a.ctypes.data, PV.IN_WORDS, out.ctypes.data, PV.OUT_WORDS, 1) != 0  # past the last op
