"""GPU parity tests for the BATCHED multiexp (mi355zk_bn254_g{1,2}_msm_batch_dev, include/mi355zk.h): B exponent vectors over one base vector
and one density map in one pipeline.  The contract is the single call: vector v of a batch returns what mi355zk_bn254_g{1,2}_msm_ex_dev returns
for it alone -- return code, error index and point -- and, for n <= 4097, what the CPU oracle computes.  Points are compared as affine records
(mi355zk_bn254_g{1,2}_to_affine), never as Jacobian words."""
import ctypes as C

import numpy as np
import pytest

import bn254_model as M
import golden_util as GU
import inputs
import oracle_lib as O

pytestmark = pytest.mark.gpu

R_MINUS_1 = np.array(M.to_limbs(M.R_ORDER - 1), dtype=np.uint64)
ONE = np.array([1, 0, 0, 0], dtype=np.uint64)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def _dev(arr):
    import torch

    arr = np.ascontiguousarray(arr)
    return torch.from_numpy((arr if arr.flags.writeable else arr.copy()).view(np.int64)).cuda()


def _affine(zk, group, jac):
    out = np.zeros(8 * group, dtype=np.uint64)
    fn = zk.lib.load().mi355zk_bn254_g1_to_affine if group == 1 else zk.lib.load().mi355zk_bn254_g2_to_affine
    assert fn(_vp(out), _vp(np.ascontiguousarray(jac, dtype=np.uint64))) == 0
    return out


def _density_args(bits):
    if bits is None:
        return None, 0, None
    words = np.ascontiguousarray(GU.density_words(bits), dtype=np.uint32)
    return _vp(words), len(bits), words   # (the array is returned to keep it alive)


def _single(zk, group, d_bases, n_bases, offset, d_vec, n, bits=None, flags=0):
    """mi355zk_bn254_g{1,2}_msm_ex_dev(..., flags, 1, 0, ...) on one vector: (rc, error index, Jacobian words)"""
    import torch

    lib = zk.lib.load()
    out = np.zeros(12 * group, dtype=np.uint64)
    dp, dbits, keep = _density_args(bits)
    fn = lib.mi355zk_bn254_g1_msm_ex_dev if group == 1 else lib.mi355zk_bn254_g2_msm_ex_dev
    rc = fn(C.c_void_p(d_bases.data_ptr()), n_bases, offset, C.c_void_p(d_vec.data_ptr()), n, dp, dbits, flags, 1, 0, None, _vp(out))
    idx = int(lib.mi355zk_last_error_index()) if rc != 0 else -1
    torch.cuda.synchronize()
    return rc, idx, out


def _batch(zk, group, d_bases, n_bases, offset, d_scalars, n, stride, n_vectors, bits=None, flags=0):
    lib = zk.lib.load()
    out = np.zeros((n_vectors, 12 * group), dtype=np.uint64)
    rcs = np.full(n_vectors, -77, dtype=np.int32)
    idxs = np.full(n_vectors, -77, dtype=np.int64)
    dp, dbits, keep = _density_args(bits)
    fn = lib.mi355zk_bn254_g1_msm_batch_dev if group == 1 else lib.mi355zk_bn254_g2_msm_batch_dev
    rc = fn(C.c_void_p(d_bases.data_ptr()), n_bases, offset, C.c_void_p(d_scalars.data_ptr()), n, stride, n_vectors, dp, dbits, flags, None, _vp(out),
            _vp(rcs), _vp(idxs))
    return rc, rcs, idxs, out


def _check_against_single_calls(zk, group, bases, vectors, stride=None, offset=0, bits=None, flags=0, oracle=None, n_bases=None):
    """vectors: (B, n, 4) u64 host array.  Every vector of the batch against its single call (rc, index, affine point); returns the affine points."""
    import torch

    n_vec, n = vectors.shape[0], vectors.shape[1]
    stride = n if stride is None else stride
    n_bases = bases.shape[0] if n_bases is None else n_bases
    d_bases = _dev(bases)
    flat = np.empty((n_vec * stride + 1, 4), dtype=np.uint64)
    flat[:] = np.uint64(0xFFFFFFFFFFFFFFFF)   # what lies between two vectors is not read: not even canonical
    for v in range(n_vec):
        flat[v * stride:v * stride + n] = vectors[v]
    d_flat = _dev(flat)
    rc, rcs, idxs, out = _batch(zk, group, d_bases, n_bases, offset, d_flat, n, stride, n_vec, bits, flags)
    torch.cuda.synchronize()
    assert rc == 0
    points = []
    for v in range(n_vec):
        d_vec = _dev(vectors[v]) if n else d_flat
        s_rc, s_idx, s_out = _single(zk, group, d_bases, n_bases, offset, d_vec, n, bits, flags)
        assert (int(rcs[v]), int(idxs[v])) == (s_rc, s_idx), (v, rcs, idxs)
        if s_rc == 0:
            got = _affine(zk, group, out[v])
            assert np.array_equal(got, _affine(zk, group, s_out)), v
            points.append(got)
        else:
            points.append(None)
    if oracle is not None:
        G = O.G1 if group == 1 else O.G2
        for v in range(n_vec):
            o_rc, want = G.multiexp(bases, oracle[v], density=None if bits is None else GU.density_words(bits), density_bits=None if bits is None else len(bits),
                                    base_offset=offset, threads=8)
            assert o_rc == 0 and np.array_equal(points[v], G.to_affine(want)), v
    return points


_bases_cache = {}


def _bases(group, n):
    """one base vector per group, computed once and shared: the tests slice it and leave it unchanged"""
    top = (1 << 14) + 8 if group == 1 else (1 << 12) + 8
    if group not in _bases_cache:
        b = inputs.bases_progression_cpu(group, top, seed=8800 + group)
        b.setflags(write=False)
        _bases_cache[group] = b
    assert n <= top
    return _bases_cache[group][:n]


CASES = [(1, n, b) for n in (1, 5, 33, 1000, 4097, 1 << 14) for b in (1, 2, 3, 16)] + [(2, n, b) for n in (1, 33, 1000, 1 << 12) for b in (1, 3, 8)]


@pytest.mark.parametrize("group,n,n_vec", CASES, ids=["g%d-n%d-B%d" % c for c in CASES])
def test_every_vector_equals_its_single_call_and_the_oracle(zk, worker, group, n, n_vec):
    bases = _bases(group, n)
    vectors = inputs.random_scalars(n_vec * n, seed=8900 + 31 * n + n_vec).reshape(n_vec, n, 4)
    _check_against_single_calls(zk, group, bases, vectors, oracle=vectors if n <= 4097 else None)


def test_scalars_that_separate_the_vectors(zk, worker):
    """an all-zero vector among random ones (the identity), a 0/1 witness-like vector (its heavy buckets exist in that vector only), a vector of
    r - 1, two equal vectors, and a stride of n + 7 with garbage between the vectors"""
    n = 3000
    bases = _bases(1, n)
    rnd = inputs.random_scalars(3 * n, seed=9001).reshape(3, n, 4)
    zero = np.zeros((n, 4), dtype=np.uint64)
    witness = np.zeros((n, 4), dtype=np.uint64)
    witness[:, 0] = np.random.default_rng(9002).integers(0, 2, size=n, dtype=np.uint64)
    top = np.tile(R_MINUS_1, (n, 1))
    vectors = np.stack([rnd[0], zero, witness, rnd[1], top, rnd[0], rnd[2]])
    points = _check_against_single_calls(zk, 1, bases, vectors, stride=n + 7, oracle=vectors)
    assert not points[1].any()                                        # the identity
    assert np.array_equal(points[0], points[5]) and not np.array_equal(points[0], points[3])
    # sum of r - 1 over all bases = -(sum of the bases): the witness-like and the top vector did not borrow each other's buckets
    rc, want = O.G1.multiexp(bases, np.tile(ONE, (n, 1)), threads=8)
    neg = O.G1.to_affine(want).copy()
    y = sum(int(v) << (64 * i) for i, v in enumerate(neg[4:8]))       # (a Montgomery form negates like the value it stands for)
    neg[4:8] = np.array(M.to_limbs((M.Q - y) % M.Q), dtype=np.uint64)
    assert rc == 0 and np.array_equal(points[4], neg)


@pytest.mark.parametrize("group", [1, 2])
def test_shared_density_map_with_a_base_offset(zk, worker, group):
    n, n_vec, offset = 1000, 3, 5
    bits = np.random.default_rng(9100 + group).random(n) < 0.55
    bases = _bases(group, int(bits.sum()) + offset)
    vectors = inputs.random_scalars(n_vec * n, seed=9101 + group).reshape(n_vec, n, 4)
    vectors[1, ::13] = 0
    vectors[2, 3::7] = ONE
    _check_against_single_calls(zk, group, bases, vectors, offset=offset, bits=bits, oracle=vectors)


@pytest.mark.parametrize("group", [1, 2])
def test_montgomery_scalars_against_canonical_ones(zk, worker, group):
    n, n_vec = 1000, 3
    bases = _bases(group, n)
    canon = inputs.random_scalars(n_vec * n, seed=9200 + group).reshape(n_vec, n, 4)
    canon[0, 0] = 0
    canon[1, 1] = ONE
    canon[2, 2] = R_MINUS_1
    r2 = np.array(M.to_limbs(pow(2, 512, M.R_ORDER)), dtype=np.uint64)
    mont = O.fe_mul_many(O.FR, canon.reshape(-1, 4), np.tile(r2, (n_vec * n, 1))).reshape(n_vec, n, 4)
    a = _check_against_single_calls(zk, group, bases, mont, flags=zk.lib.MSM_SCALARS_MONTGOMERY, oracle=canon)
    b = _check_against_single_calls(zk, group, bases, canon)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


def test_several_passes(zk, worker):
    """n = 64 with more vectors than one pipeline pass holds bucket sets for: the pass size from the diagnostic export"""
    lib = zk.lib.load()
    n = 64
    cap, w, per = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert lib.mi355zk_msm_batch_geometry(n, 1 << 20, 1, C.byref(cap), C.byref(w), C.byref(per)) == 0
    assert per.value == cap.value // w.value and per.value >= 2     # bucket sets, not memory, bound a pass of 64-exponent vectors
    n_vec = per.value + 3                                           # a full pass and a short one
    assert n_vec * w.value > cap.value
    assert lib.mi355zk_msm_batch_geometry(n, n_vec, 1, None, None, C.byref(per)) == 0 and per.value == cap.value // w.value
    vectors = inputs.random_scalars(n_vec * n, seed=9300).reshape(n_vec, n, 4)
    vectors[per.value - 1, :] = 0                                   # the last vector of the first pass and the first of the second one
    vectors[per.value, :, 1:] = 0
    points = _check_against_single_calls(zk, 1, _bases(1, n), vectors)
    assert not points[per.value - 1].any() and len({p.tobytes() for p in points}) == n_vec
    # a lone last vector takes the single call
    _check_against_single_calls(zk, 1, _bases(1, n), vectors[:per.value + 1])


def test_errors_are_those_of_the_single_calls(zk, worker):
    n, n_vec = 500, 4
    bases = _bases(1, n).copy()
    bases[100] = 0                                                  # an identity base ...
    bases[7] = 0
    vectors = inputs.random_scalars(n_vec * n, seed=9400).reshape(n_vec, n, 4)
    vectors[:, 7] = 0                                               # (under a zero exponent in every vector: never looked at)
    vectors[0, 100] = 0
    vectors[2, 100] = 0
    vectors[3, 100] = 0                                             # ... under a non-zero exponent of vector 1 only
    pts = _check_against_single_calls(zk, 1, bases, vectors)
    assert [p is None for p in pts] == [False, True, False, False]
    lib = zk.lib.load()
    rc, rcs, idxs, _ = _batch(zk, 1, _dev(bases), n, 0, _dev(vectors.reshape(-1, 4)), n, n, n_vec)
    assert rc == 0 and list(rcs) == [0, zk.lib.ERR_UNEXPECTED_IDENTITY, 0, 0] and list(idxs) == [-1, 100, -1, -1]
    # a non-canonical exponent in vector 2 only
    bad = inputs.random_scalars(n_vec * n, seed=9401).reshape(n_vec, n, 4)
    bad[2, 321, 3] = np.uint64(1 << 62)
    pts = _check_against_single_calls(zk, 1, _bases(1, n), bad)
    assert [p is None for p in pts] == [False, False, True, False]
    rc, rcs, idxs, _ = _batch(zk, 1, _dev(_bases(1, n)), n, 0, _dev(bad.reshape(-1, 4)), n, n, n_vec)
    assert rc == 0 and list(rcs) == [0, 0, zk.lib.ERR_BAD_ARGS, 0] and list(idxs) == [-1, -1, 321, -1]
    # both at once, and a density map in front: the identity base belongs to the 3rd selected exponent
    bits = np.ones(n, dtype=bool)
    bits[1] = False
    b2 = _bases(1, n).copy()
    b2[2] = 0
    _check_against_single_calls(zk, 1, b2, bad, bits=bits)
    # exponents beyond the bases: UnexpectedEof for every vector, unless it has an earlier error of its own
    short = _bases(1, n - 10).copy()
    short[100] = 0
    pts = _check_against_single_calls(zk, 1, short, vectors)
    assert all(p is None for p in pts)
    rc, rcs, idxs, _ = _batch(zk, 1, _dev(short), n - 10, 0, _dev(vectors.reshape(-1, 4)), n, n, n_vec)
    eof = zk.lib.ERR_UNEXPECTED_EOF
    assert rc == 0 and list(rcs) == [eof, zk.lib.ERR_UNEXPECTED_IDENTITY, eof, eof] and list(idxs) == [n - 10, 100, n - 10, n - 10]
    assert lib.mi355zk_last_error_index() == n - 10


def test_call_level_refusals_and_edges(zk, worker):
    import torch

    lib = zk.lib.load()
    n, n_vec = 40, 3
    d_bases = _dev(_bases(1, n))
    d_sc = _dev(inputs.random_scalars(n_vec * n, seed=9500))
    out = np.zeros((n_vec, 12), dtype=np.uint64)
    rcs = np.zeros(n_vec, dtype=np.int32)
    idxs = np.zeros(n_vec, dtype=np.int64)
    fn = lib.mi355zk_bn254_g1_msm_batch_dev
    b, s = C.c_void_p(d_bases.data_ptr()), C.c_void_p(d_sc.data_ptr())
    bad = zk.lib.ERR_BAD_ARGS
    assert fn(b, n, 0, s, n, n, n_vec, None, 0, 0, None, None, _vp(rcs), _vp(idxs)) == bad          # NULL outputs
    assert fn(b, n, 0, s, n, n, n_vec, None, 0, 0, None, _vp(out), None, _vp(idxs)) == bad
    assert fn(b, n, 0, s, n, n, n_vec, None, 0, 0, None, _vp(out), _vp(rcs), None) == bad
    assert fn(None, n, 0, s, n, n, n_vec, None, 0, 0, None, _vp(out), _vp(rcs), _vp(idxs)) == bad       # NULL inputs with a count
    assert fn(b, n, 0, None, n, n, n_vec, None, 0, 0, None, _vp(out), _vp(rcs), _vp(idxs)) == bad
    assert fn(b, n, 0, s, n, n, 0, None, 0, 0, None, _vp(out), _vp(rcs), _vp(idxs)) == bad              # no vector
    assert fn(b, n, 0, s, n, n - 1, n_vec, None, 0, 0, None, _vp(out), _vp(rcs), _vp(idxs)) == bad      # stride < n
    assert fn(b, n, 0, s, n, n, n_vec, None, 0, 2, None, _vp(out), _vp(rcs), _vp(idxs)) == bad          # unknown flag
    assert fn(b, 1 << 31, 0, s, n, n, n_vec, None, 0, 0, None, _vp(out), _vp(rcs), _vp(idxs)) == bad    # sizes >= 2^31
    assert fn(b, n, 0, s, 1 << 31, 1 << 31, n_vec, None, 0, 0, None, _vp(out), _vp(rcs), _vp(idxs)) == bad
    assert fn(b, n, 0, s, n, n, 1 << 31, None, 0, 0, None, _vp(out), _vp(rcs), _vp(idxs)) == bad
    assert lib.mi355zk_bn254_g2_msm_batch_dev(b, n, 0, s, n, n, 0, None, 0, 0, None, _vp(out), _vp(rcs), _vp(idxs)) == bad
    # no exponents: B identities
    out[:] = 7
    rcs[:] = 5
    assert fn(b, n, 0, None, 0, 0, n_vec, None, 0, 0, None, _vp(out), _vp(rcs), _vp(idxs)) == 0
    assert not rcs.any() and list(idxs) == [-1] * n_vec and all(not _affine(zk, 1, out[v]).any() for v in range(n_vec))
    torch.cuda.synchronize()


def test_multiexp_many_carries_what_multiexp_would(zk, worker):
    """bellman.multiexp_many over a tensor and over a window table; the futures' errors are multiexp's"""
    import torch

    n, n_vec = 1000, 3
    bases = _bases(1, n).copy()
    d_bases = _dev(bases)
    vectors = inputs.random_scalars(n_vec * n, seed=9600).reshape(n_vec, n, 4)
    d_vec = _dev(vectors.reshape(-1, 4)).reshape(n_vec, n, 4)
    table = zk.MsmTable(d_bases)
    for src in (d_bases, table):
        futs = zk.multiexp_many(worker, (src, 0), zk.FullDensity(), d_vec)
        assert len(futs) == n_vec
        for v, f in enumerate(futs):
            want = zk.multiexp(worker, (src, 0), zk.FullDensity(), d_vec[v].contiguous()).wait()
            assert np.array_equal(_affine(zk, 1, f.wait()), _affine(zk, 1, want))
    bases[10] = 0
    d_bad = _dev(bases)
    futs = zk.multiexp_many(worker, (d_bad, 0), zk.FullDensity(), d_vec)
    for f in futs:
        with pytest.raises(zk.SynthesisError) as e:
            f.wait()
        assert e.value.kind == zk.SynthesisError.UNEXPECTED_IDENTITY and e.value.index == 10
    vectors[1, 10] = 0
    futs = zk.multiexp_many(worker, (d_bad, 0), zk.FullDensity(), _dev(vectors.reshape(-1, 4)).reshape(n_vec, n, 4))
    futs[1].wait()
    with pytest.raises(zk.SynthesisError):
        futs[0].wait()
    torch.cuda.synchronize()
