"""KZG in evaluation form (phase2-bn254_amd/kzg.py: srs_lagrange, commit_evals, open_evals) over a small accumulator: the commitments and
proofs are the records that commit / open give for the same polynomial in coefficient form, for points outside and inside the domain; the
pairing check accepts them and refuses each tampered opening; infinity stays a valid commitment and a valid proof."""
import numpy as np
import pytest

import bn254_model as M
import fixed_base_cases as FB
import fr_poly_cases as P
import oracle_lib as O
from test_gpu_kzg import ALPHA, BETA, TAU, Z, coeffs_dev, g1_mul, poly, proof_scalar

pytestmark = pytest.mark.gpu

R = M.R_ORDER
LOG_N = 4
N = 1 << LOG_N
OMEGA = pow(M.FR_ROOT_OF_UNITY, 1 << (M.FR_S - LOG_N), R)


@pytest.fixture(scope="module")
def srs(zk, worker):
    acc = zk.ceremony.contribute_accumulator(zk.ceremony.new_accumulator(LOG_N, "cuda"), TAU, ALPHA, BETA)
    return zk.kzg.srs_from_accumulator(acc)


@pytest.fixture(scope="module")
def lsrs(zk, srs):
    before = srs["g1"].clone()
    out = zk.kzg.srs_lagrange(srs, LOG_N)
    assert out["log_n"] == LOG_N and out["g1_lagrange"].shape == (N, 8) and out["g1"] is srs["g1"]
    assert bool((srs["g1"] == before).all())   # the powers themselves are not transformed
    return out


def evals_dev(zk, worker, p):
    """the evaluations over the domain of the polynomial with the coefficients p (len(p) <= N)"""
    dom = zk.EvaluationDomain(coeffs_dev(list(p) + [0] * (N - len(p))), LOG_N)
    dom.fft(worker)
    return dom.into_coeffs()


@pytest.mark.parametrize("n_coeffs", [N, N - 1, 10, 2])
def test_commitments_are_those_of_the_coefficient_form(zk, worker, srs, lsrs, n_coeffs):
    K = zk.kzg
    p = poly(n_coeffs)
    c = K.commit_evals(lsrs, evals_dev(zk, worker, p))
    assert np.array_equal(c, K.commit(srs, coeffs_dev(p))) and np.array_equal(c, g1_mul(P.horner(p, TAU)))


@pytest.mark.parametrize("z", [Z, 0, 1, OMEGA, R - 1, pow(OMEGA, N - 1, R)], ids=["random", "zero", "one", "omega", "omega^(n/2)", "omega^(n-1)"])
def test_openings_are_those_of_the_coefficient_form_and_check(zk, worker, srs, lsrs, z):
    K = zk.kzg
    p = poly(N, seed=5)
    d, e = coeffs_dev(p), evals_dev(zk, worker, p)
    c = K.commit_evals(lsrs, e)
    value, proof = K.open_evals(lsrs, e, z)
    want_value, want_proof = K.open(srs, d, z)
    assert value == want_value == P.horner(p, z)
    assert np.array_equal(proof, want_proof) and np.array_equal(proof, g1_mul(proof_scalar(p, z)))
    assert K.evaluate_evals(e, [z]) == [value]
    assert K.check(srs, c, z, value, proof) is True
    assert K.check(srs, c, z, (value + 1) % R, proof) is False
    assert K.check(srs, c, (z + 1) % R, value, proof) is False
    assert K.check(srs, c, z, value, g1_mul(5)) is False
    assert K.check(srs, O.G1.mul_many_affine(c, FB.limbs([2]))[0], z, value, proof) is False


def test_infinity_is_a_valid_proof_and_a_valid_commitment(zk, worker, srs, lsrs):
    K = zk.kzg
    e = evals_dev(zk, worker, [12345])                       # a constant: the same value at every point of the domain
    assert np.array_equal(P.ints(e.cpu().numpy()), [12345 * P.MONT % R] * N)
    c = K.commit_evals(lsrs, e)
    for z in (Z, OMEGA):
        value, proof = K.open_evals(lsrs, e, z)
        assert value == 12345 and not proof.any() and np.array_equal(c, g1_mul(12345))
        assert K.check(srs, c, z, value, proof) is True
        assert K.check(srs, c, z, 12346, proof) is False
    e = evals_dev(zk, worker, [0] * N)                       # the zero polynomial
    c = K.commit_evals(lsrs, e)
    for z in (Z, 1):
        value, proof = K.open_evals(lsrs, e, z)
        assert value == 0 and not c.any() and not proof.any()
        assert K.check(srs, c, z, 0, proof) is True
        assert K.check(srs, c, z, 1, proof) is False


def test_batched_forms_equal_the_loops(zk, worker, srs, lsrs):
    import torch

    K = zk.kzg
    p = poly(N, seed=6)
    e = evals_dev(zk, worker, p)
    zs = [Z, 0, OMEGA, 1, R - 1, Z]
    values, proofs = K.open_evals_many(lsrs, e, zs)
    assert proofs.shape == (len(zs), 8)
    for j, z in enumerate(zs):
        v, w = K.open_evals(lsrs, e, z)
        assert values[j] == v == P.horner(p, z) and np.array_equal(proofs[j], w)
    commitments = np.tile(K.commit_evals(lsrs, e), (len(zs), 1))
    assert K.check_many(srs, commitments, zs, values, proofs).tolist() == [True] * len(zs)
    many = torch.stack([evals_dev(zk, worker, poly(N, seed=s)) for s in range(3)])
    got = K.commit_evals_many(lsrs, many)
    for s in range(3):
        assert np.array_equal(got[s], K.commit_evals(lsrs, many[s]))


def test_the_wrong_srs_is_refused(zk, worker, srs, lsrs):
    K = zk.kzg
    with pytest.raises(ValueError):
        K.srs_lagrange(srs, LOG_N + 1)                       # the accumulator holds 2^(LOG_N + 1) - 1 powers
    e = evals_dev(zk, worker, poly(N))
    with pytest.raises(ValueError):
        K.commit_evals(srs, e)                               # no Lagrange basis
    with pytest.raises(ValueError):
        K.commit_evals(lsrs, e[:N // 2])                     # another domain
    with pytest.raises(ValueError):
        K.open_evals(lsrs, e[:N // 2], Z)
    with pytest.raises(ValueError):
        K.commit_evals(lsrs, e[:N - 1])                      # not a domain at all
