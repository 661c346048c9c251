"""The point-FFT edge table (tests/point_fft_edge_inputs.py) proven on the CPU: every vector's closed form against the oracle's
EvaluationDomain<Point<G>>::{fft, ifft} + batch_normalization, ifft(fft(v)) == v through the oracle, the big-int side of the table against
the oracle's scalar multiplication, and -- restated as assertions on the scalars -- what each family makes the butterflies of
pfft_stage_kernel (G1 and G2 instances) meets.  tests/test_gpu_point_fft_edges.py runs the same table on the device."""
import numpy as np
import pytest

import bn254_model as M
import inputs
import oracle_lib as O
import point_fft_edge_inputs as T

R = M.R_ORDER
SIZES = [(g, l) for g in (1, 2) for l in T.LOG_N[g]]
CASES = [(g, l, name) for g, l in SIZES for name in T.names(g, l)]
OPS = ("fft", "ifft")


def _ids(c):
    return "G%d-2^%d-%s" % c if len(c) == 3 else "G%d-2^%d" % c


@pytest.mark.parametrize("group", [1, 2])
def test_base_point_and_the_fixed_base_multiples(group):
    """P is base_scalar * generator by the big-int double-and-add as well, lies on its curve, and the table's fixed-base multiples agree with
    the plain big-int multiplication and with the oracle's on 0, 1, 2, r - 1, a domain size and random scalars."""
    F = M.FQ_OPS if group == 1 else M.FQ2_OPS
    gen = M.G1_GEN if group == 1 else M.G2_GEN
    G = O.G1 if group == 1 else O.G2
    P = T._from_raw(group, T.base_point_raw(group))
    assert P == M.ec_mul(F, gen, T.base_scalar(group))
    assert (M.on_curve_g1 if group == 1 else M.on_curve_g2)(P)
    assert M.ec_mul(F, P, R) is None                                   # order r
    ks = [0, 1, 2, R - 1, 512, R + 3] + [M.from_limbs(k) for k in inputs.random_scalars(6, seed=77)]
    for k in ks:
        assert list(T.multiple_raw(group, k)) == T._to_raw(group, M.ec_mul(F, P, k % R)), hex(k)
    by_oracle = G.mul_many_affine(T.base_point_raw(group), np.array([M.to_limbs(k % R) for k in ks], dtype=np.uint64))
    assert np.array_equal(by_oracle, np.array([T.multiple_raw(group, k) for k in ks], dtype=np.uint64))
    assert not by_oracle[0].any()
    assert np.array_equal(T.negate_records(group, by_oracle[1:2])[0], by_oracle[3])     # -P == (r - 1) P


@pytest.mark.parametrize("log_n", range(0, 10))
@pytest.mark.parametrize("inverse", [False, True])
def test_butterflies_replays_the_transform(log_n, inverse):
    """the scalar replay of the kernels' network computes the DFT of domain.rs (against bn254_model.domain_op), so what the purpose tests below
    read off its trace is what the butterflies of a correct transform meet"""
    a = [M.from_limbs(k) for k in inputs.random_fr_mont(1 << log_n, seed=500 + log_n)]
    trace, out = T.butterflies(a, log_n, inverse)
    assert out == M.domain_op(a, "ifft" if inverse else "fft")
    assert len(trace) == log_n << log_n >> 1
    assert all(w == 1 for s, j, u, w, t in trace if j == 0) and all(w != 1 for s, j, u, w, t in trace if j != 0)


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_vector_closed_form_oracle_and_roundtrip(case):
    group, log_n, name = case
    v = T.vector(group, log_n, name)
    n = v.n
    if v.scalars is not None:
        # the input records by the big-int model, independent of the oracle that made them
        assert np.array_equal(v.points, T.records_of(group, {i: s for i, s in enumerate(v.scalars) if s % R}, n))
    for op in OPS:
        want = T.oracle(group, log_n, name, op)
        assert want.shape == v.points.shape
        if v.closed is not None:
            # the closed form is the DFT of the scalars (big ints) ...
            dft = M.domain_op([s % R for s in v.scalars], op)
            assert {j: s for j, s in enumerate(dft) if s} == {j: s % R for j, s in v.closed[op].items()}, op
            # ... and its records are the oracle's, byte for byte
            assert np.array_equal(v.expect(op), want), op
    back = O.point_domain_op(group, T.oracle(group, log_n, name, "fft"), log_n, "ifft")
    assert np.array_equal(back, v.points)
    back = O.point_domain_op(group, T.oracle(group, log_n, name, "ifft"), log_n, "fft")
    assert np.array_equal(back, v.points)


# ------------------------------------------------------------------------------------------------ what each family is there for
def _traces(v):
    return [T.butterflies(v.scalars, v.log_n, inv)[0] for inv in (False, True)]


@pytest.mark.parametrize("size", SIZES, ids=_ids)
def test_constant_doubles_and_cancels_at_stage_0(size):
    """v_i = P: every stage-0 butterfly is P + P (the doubling branch under a unit twiddle) and P - P (infinity); n P at index 0 is the only output"""
    v = T.vector(*size, "constant")
    assert v.points.any(axis=1).all() and (v.points == v.points[0]).all()
    for trace in _traces(v):
        st0 = [b for b in trace if b[0] == 0]
        assert len(st0) == v.n // 2 and all(u == t == 1 and w == 1 for s, j, u, w, t in st0)
        # and so on: the unit-twiddle butterfly of every block doubles 2^s P, every other one has both operands infinite
        assert all((u == t == 1 << s) if j == 0 else (u == t == 0) for s, j, u, w, t in trace)
    assert list(v.closed["fft"]) == [0] and list(v.closed["ifft"]) == [0]


@pytest.mark.parametrize("size", SIZES, ids=_ids)
def test_all_infinity_is_all_zero_records(size):
    v = T.vector(*size, "all_infinity")
    assert not v.points.any()
    for op in OPS:
        assert not v.expect(op).any() and not T.oracle(*size, "all_infinity", op).any()


@pytest.mark.parametrize("size", SIZES, ids=_ids)
def test_delta_meets_infinite_operands(size):
    """one P among infinities: no butterfly has two finite operands.  Stage 0 has ONE butterfly that is not infinity +- infinity: (P, infinity) for d < n/2,
    (infinity, P) -- an infinite u against a finite t under the unit twiddle -- from d = n/2 on; the last stage has an infinite operand in every butterfly, and for
    odd d it is u, with t finite under a non-unit twiddle (the whole multiplication, then infinity +- w t).  Every output is a finite omega^(+-jd) P (/ n)."""
    group, log_n = size
    n = 1 << log_n
    for name in T.closed_form_names(log_n):
        if not name.startswith("delta_"):
            continue
        v = T.vector(group, log_n, name)
        d = T._delta_positions(n)[name]
        assert [i for i in range(n) if v.points[i].any()] == [d] and np.array_equal(v.points[d], T.base_point_raw(group))
        for trace in _traces(v):
            assert all(u == 0 or t == 0 for s, j, u, w, t in trace)
            hit = [(u, t) for s, j, u, w, t in trace if s == 0 and (u or t)]
            assert hit == ([(0, 1)] if d >= n // 2 else [(1, 0)])
            assert all((u == 0) != (t == 0) for s, j, u, w, t in trace if s == log_n - 1)
            assert any(u == 0 and t == 0 for s, j, u, w, t in trace) == (n >= 4)
            assert any(u == 0 and t != 0 and w != 1 for s, j, u, w, t in trace) == (d % 2 == 1 and n >= 4)
        for op in OPS:
            assert sorted(v.closed[op]) == list(range(n)) and all(s % R for s in v.closed[op].values())
    assert "delta_half" in T.closed_form_names(log_n) or n == 2


@pytest.mark.parametrize("size", SIZES, ids=_ids)
def test_frequency_butterflies_meet_equal_or_opposite_operands_at_every_stage(size):
    """v_i = omega^(ik) P: every sub-transform is a single frequency again, so EVERY butterfly of EVERY stage has u == w t (u + w t doubles, u - w t
    is infinity) or u == -w t, or both operands infinite -- under non-unit twiddles from stage 1 on, with w t the result of the windowed
    multiplication.  One output is not infinity: index n - k (fft), index k (ifft)."""
    group, log_n = size
    n = 1 << log_n
    names = [x for x in T.closed_form_names(log_n) if x.startswith("frequency_")]
    assert "frequency_1" in names and (n < 8 or len(names) == 4)
    for name in names:
        v = T.vector(group, log_n, name)
        k = T._frequencies(n)[name]
        assert v.points.any(axis=1).all()
        if k == n // 2:   # the alternating vector P, -P
            assert np.array_equal(v.points[0::2], np.tile(T.base_point_raw(group), (n // 2, 1)))
            assert np.array_equal(v.points[1::2], T.negate_records(group, v.points[0::2]))
        for trace in _traces(v):
            same = opposite = nonunit = 0
            for s, j, u, w, t in trace:
                wt = w * t % R
                assert (u == 0 and t == 0) or (u != 0 and (u == wt or (u + wt) % R == 0)), (name, s, j)
                same += u != 0 and u == wt
                opposite += u != 0 and (u + wt) % R == 0
                nonunit += u != 0 and w != 1
            assert same + opposite == n - 1 and (nonunit > 0) == (n >= 4 and k != n // 2)   # (k = n/2: equal operands under unit twiddles only)
            assert all(u != 0 for s, j, u, w, t in trace if s == 0)
        assert list(v.closed["fft"]) == [(n - k) % n] and list(v.closed["ifft"]) == [k]
        for op in OPS:
            out = v.expect(op)
            assert int(out.any(axis=1).sum()) == 1


@pytest.mark.parametrize("size", SIZES, ids=_ids)
def test_two_frequencies_is_a_doubled_frequency_on_even_indices(size):
    group, log_n = size
    v = T.vector(group, log_n, "two_frequencies")
    n, k = v.n, 5 % v.n
    assert v.points[0::2].any(axis=1).all() and not v.points[1::2].any()
    assert np.array_equal(v.points[0], np.array(T.multiple_raw(group, 2), dtype=np.uint64))
    for trace in _traces(v):
        for s, j, u, w, t in trace:
            wt = w * t % R
            assert t == 0 or (u != 0 and (u == wt or (u + wt) % R == 0))
        assert sum(1 for s, j, u, w, t in trace if u and t) == (n // 2 - 1 if n >= 4 else 0)
    assert sorted(v.closed["fft"]) == sorted({(n - k) % n, (n // 2 - k) % n}) and sorted(v.closed["ifft"]) == sorted({k, (k + n // 2) % n})


@pytest.mark.parametrize("size", [(g, l) for g in (1, 2) for l in T.LOG_N_ORACLE_ONLY[g]], ids=_ids)
def test_oracle_only_families_have_the_stated_shape(size):
    """mirrored_progression: distinct points below n/2; the stage-0 partner v[i + n/2] is v[i] on even i (a doubling, and a cancellation in u - t) and -v[i]
    on odd i (the other way round) -- the sums that survive are distinct doubles, so the later stages are generic.  half_infinite_*: one half infinity."""
    group, log_n = size
    h = 1 << (log_n - 1)
    v = T.vector(group, log_n, "mirrored_progression")
    lo, hi = v.points[:h], v.points[h:]
    assert lo.any(axis=1).all() and len({r.tobytes() for r in lo}) == h
    assert np.array_equal(hi[0::2], lo[0::2]) and np.array_equal(hi[1::2], T.negate_records(group, lo[1::2]))
    assert not np.array_equal(hi[1::2], lo[1::2])
    a, b = T.vector(group, log_n, "half_infinite_low"), T.vector(group, log_n, "half_infinite_high")
    assert not a.points[:h].any() and a.points[h:].any(axis=1).all()
    assert b.points[:h].any(axis=1).all() and not b.points[h:].any()
    for x in (v, a, b):
        assert x.closed is None and x.expect("fft") is None
        for op in OPS:
            assert T.oracle(group, log_n, x.name, op).any()


@pytest.mark.parametrize("group", [1, 2])
def test_small_sizes_give_whole_normalisation_groups_of_infinity(group):
    """batch_normalize_kernel shares one inversion among K consecutive records: at n < K the one group is partly (frequency, constant) or wholly
    (all_infinity) made of Z == 0, and from n = 2 K on `frequency` leaves whole groups of K infinities next to the group with its one point."""
    K = T.NORMALISE_GROUP[group]
    small = [l for l in T.LOG_N[group] if (1 << l) < K]
    assert small == list(range(1, K.bit_length() - 1)) and len(small) >= 2
    for l in T.LOG_N[group]:
        n = 1 << l
        for name in T.closed_form_names(l):
            if name.startswith("frequency_") or name in ("constant", "all_infinity", "two_frequencies"):
                for op in OPS:
                    out = T.vector(group, l, name).expect(op)
                    zero_groups = [g for g in range(0, n, K) if not out[g:g + K].any()]
                    finite = int(out.any(axis=1).sum())
                    assert finite == len(T.vector(group, l, name).closed[op])
                    assert len(zero_groups) >= (n + K - 1) // K - finite
                    if name == "all_infinity" or n >= 4 * K:
                        assert zero_groups
