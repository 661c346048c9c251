"""The point FFTs on the device against the edge table of tests/point_fft_edge_inputs.py (proven on the CPU by test_point_fft_edges_host.py):
vectors of multiples of one point, on which the butterflies of pfft_stage_kernel (G1 and G2 instances) meet equal operands (the doubling branch of
jacu_add_tab / jacu2_add_tab behind a 33- or 64-window multiplication), opposite ones, infinite u or t under unit and non-unit twiddles, and leave
whole normalisation groups of infinities -- every record of every vector byte for byte against the oracle's Point<G> FFT + batch_normalization, against
the big-int closed form where the family has one, and fft(ifft(v)) == v == ifft(fft(v)).  G1 at every log_n of 1..9, G2 at 1..7 through the plain windows and
the psi split.  Then the launch loop of point_fft_g1 / point_fft_g2 cut by MI355ZK_PFFT_CHUNK_TEST into several (ragged) launches per stage."""
import ctypes as C
import functools

import numpy as np
import pytest

import inputs
import oracle_lib as O
import point_fft_edge_inputs as T

pytestmark = pytest.mark.gpu

OPS = ("fft", "ifft")
G1_CASES = [(l, name) for l in T.LOG_N[1] for name in T.names(1, l)]
G2_CASES = [(l, name) for l in T.LOG_N[2] for name in T.names(2, l)]


def _id(c):
    return "2^%d-%s" % c


def _run(zk, pts, log_n, mode, group):
    import torch

    d = torch.from_numpy(np.ascontiguousarray(pts).view(np.int64)).cuda()
    fn = zk.lib.load().mi355zk_bn254_g1_point_fft_dev if group == 1 else zk.lib.load().mi355zk_bn254_g2_point_fft_dev
    assert fn(C.c_void_p(d.data_ptr()), log_n, mode, None) == 0
    return d.cpu().numpy().view(np.uint64)


def _check_vector(zk, group, log_n, name, trusted):
    v = T.vector(group, log_n, name)
    got = {}
    for op in OPS:
        got[op] = _run(zk, v.points, log_n, (1 if op == "ifft" else 0) | trusted, group)
        bad = np.flatnonzero((got[op] != T.oracle(group, log_n, name, op)).any(axis=1))
        assert bad.size == 0, "%s of %r: records %s differ from the oracle" % (op, v, bad[:8])
        want = v.expect(op)
        if want is not None:
            assert np.array_equal(got[op], want), op
            if name == "all_infinity" or name.startswith("frequency_") or name == "constant":
                # whole groups of the shared inversion with Z == 0 (every record of it at n below the group size): all-zero records, stated outright
                finite = sorted(v.closed[op])
                assert len(finite) <= 1 and np.flatnonzero(got[op].any(axis=1)).tolist() == finite
    assert np.array_equal(_run(zk, got["ifft"], log_n, 0 | trusted, group), v.points), "fft(ifft(v)) != v"
    assert np.array_equal(_run(zk, got["fft"], log_n, 1 | trusted, group), v.points), "ifft(fft(v)) != v"


@pytest.mark.parametrize("case", G1_CASES, ids=_id)
def test_g1_point_fft_on_the_edge_table(zk, worker, case):
    _check_vector(zk, 1, case[0], case[1], 0)


@pytest.mark.parametrize("case", G2_CASES, ids=_id)
@pytest.mark.parametrize("trusted", [0, 2], ids=["plain", "psi_split"])
def test_g2_point_fft_on_the_edge_table(zk, worker, case, trusted):
    """mode 0 (64 plain windows) and, the table being multiples of a subgroup point, MI355ZK_G2_TRUSTED_SUBGROUP (33 windows split over psi)"""
    _check_vector(zk, 2, case[0], case[1], trusted)


# ------------------------------------------------------------------------------------------------ the launch loop in chunks
@functools.lru_cache(maxsize=None)
def _progression(group, log_n):
    """distinct points with one infinity planted (the input of test_gpu_point_fft.py's parity tests) and the oracle's two transforms of it"""
    pts = inputs.bases_progression_cpu(group, 1 << log_n, seed=0xC4 + 16 * log_n + group)
    pts[3] = 0
    pts.setflags(write=False)
    return pts, {op: O.point_domain_op(group, pts, log_n, op) for op in OPS}


def _chunk_inputs(group, log_n):
    pts, want = _progression(group, log_n)
    yield "progression", pts, want
    yield "frequency_5", T.vector(group, log_n, "frequency_5").points, {op: T.oracle(group, log_n, "frequency_5", op) for op in OPS}


CHUNKED = [(1, 8, 48, 0), (2, 6, 24, 0), (2, 6, 24, 2), (1, 3, 1, 0), (2, 3, 1, 0), (2, 3, 1, 2)]


@pytest.mark.parametrize("group,log_n,chunk,trusted", CHUNKED)
@pytest.mark.parametrize("op", OPS)
def test_point_fft_in_chunked_launches(zk, worker, monkeypatch, group, log_n, chunk, trusted, op):
    """MI355ZK_PFFT_CHUNK_TEST = lanes per launch.  G1 2^8 at 48: every stage is launches of 48, 48 and 32 butterflies (b0 = 0, 48, 96 over one table laid
    out with each launch's own stride), the ifft's scale pass 5 x 48 + 16 lanes; G2 2^6 at 24: 24 + 8 and 24 + 24 + 16; one lane per launch at 2^3.
    Every record against the oracle, and the array byte-equal to the same call in one launch."""
    mode = (1 if op == "ifft" else 0) | trusted
    n = 1 << log_n
    assert chunk < n // 2 and (chunk == 1 or (n // 2) % chunk)   # several launches per stage, the last one ragged
    for label, pts, want in _chunk_inputs(group, log_n):
        monkeypatch.delenv("MI355ZK_PFFT_CHUNK_TEST", raising=False)
        whole = _run(zk, pts, log_n, mode, group)
        monkeypatch.setenv("MI355ZK_PFFT_CHUNK_TEST", str(chunk))
        cut = _run(zk, pts, log_n, mode, group)
        bad = np.flatnonzero((cut != want[op]).any(axis=1))
        assert bad.size == 0, "%s, %s in launches of %d lanes: records %s differ from the oracle" % (label, op, chunk, bad[:8])
        assert np.array_equal(cut, whole), label
