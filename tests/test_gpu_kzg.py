"""KZG over tau powers (phase2-bn254_amd/kzg.py): the trapdoor being known, every commitment and proof has a closed form in the exponent --
commit = p(TAU) G, proof = q(TAU) G with q = (p - p(z)) / (x - z) -- worked out with Python big ints and the oracle's scalar
multiplication; the pairing check accepts them and refuses each tampered opening; the batched forms equal the loops byte for byte."""
import random

import numpy as np
import pytest

import bn254_model as M
import fixed_base_cases as FB
import fr_poly_cases as P
import inputs
import oracle_lib as O

pytestmark = pytest.mark.gpu

R = M.R_ORDER
TAU, ALPHA, BETA = (0x2F0E1D2C3B4A59687796A5B4C3D2E1F00F1E2D3C4B5A69788796A5B4C3D2E1F % R, 0x1B7E4D3C2A190807F6E5D4C3B2A1908F7E6D5C4B3A29180706F5E4D3C2B1A09 % R,
                    0x2468ACE013579BDF02468ACE13579BDF2468ACE013579BDF02468ACE13579BD % R)
Z = P.Z_FIXED
SIZES = ("1", "2", "64", "300", "tile+1")


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).cuda()


def g1_mul(k: int) -> np.ndarray:
    return O.G1.mul_many_affine(inputs.G1_GEN_RAW, FB.limbs([k % R]))[0]


def poly(n: int, seed: int = 0) -> list:
    rnd = random.Random(7000 + 31 * n + seed)
    return [rnd.randrange(R) for _ in range(n)]


def coeffs_dev(p):
    return dev(P.rows([c * P.MONT % R for c in p]) if p else np.zeros((0, 4), np.uint64))


def proof_scalar(p, z: int) -> int:
    """q(TAU) for q = (p - p(z)) / (x - z)"""
    return (P.horner(p, TAU) - P.horner(p, z)) * pow(TAU - z, -1, R) % R


@pytest.fixture(scope="module")
def geom(zk, worker):
    return P.geometry(zk.lib.load())


@pytest.fixture(scope="module")
def srs(zk, geom):
    """tau^i G for i <= TILE and H, tau H from the oracle's scalar multiplication"""
    powers, cur = [], 1
    for _ in range(geom[1] + 1):
        powers.append(cur)
        cur = cur * TAU % R
    g1 = O.G1.mul_many_affine(inputs.G1_GEN_RAW, FB.limbs(powers))
    g2 = O.G2.mul_many_affine(inputs.G2_GEN_RAW, FB.limbs([1, TAU]))
    return zk.kzg.srs_from_points(dev(g1), dev(g2[0]), dev(g2[1]))


def size(name: str, geom) -> int:
    return P.size(name, geom) if name in P.SIZE_NAMES else int(name)


@pytest.mark.parametrize("size_name", SIZES)
def test_commit_open_check_closed_forms_and_tampers(zk, srs, geom, size_name):
    """A constant polynomial (n = 1) takes the same value everywhere, so its opening IS valid at another point: that tamper is asserted
    for n >= 2, where it must fail."""
    K = zk.kzg
    n = size(size_name, geom)
    p = poly(n)
    d = coeffs_dev(p)
    c = K.commit(srs, d)
    assert np.array_equal(c, g1_mul(P.horner(p, TAU)))
    value, proof = K.open(srs, d, Z)
    assert value == P.horner(p, Z)
    assert K.evaluate(d, [Z, TAU]) == [P.horner(p, Z), P.horner(p, TAU)]
    assert np.array_equal(proof, g1_mul(proof_scalar(p, Z)))
    assert (n == 1) == (not proof.any())
    assert K.check(srs, c, Z, value, proof) is True
    assert K.check(srs, c, Z, (value + 1) % R, proof) is False
    assert K.check(srs, c, (Z + 1) % R, value, proof) is (n == 1)
    assert K.check(srs, c, Z, value, inputs.G1_GEN_RAW) is False
    assert K.check(srs, O.G1.mul_many_affine(c, FB.limbs([2]))[0], Z, value, proof) is False


def test_infinity_is_a_valid_proof_and_a_valid_commitment(zk, srs):
    K = zk.kzg
    d = coeffs_dev([12345])
    c = K.commit(srs, d)
    value, proof = K.open(srs, d, Z)
    assert value == 12345 and not proof.any() and np.array_equal(c, g1_mul(12345))
    assert K.check(srs, c, Z, value, proof) is True
    assert K.check(srs, c, Z, 12346, proof) is False
    d = coeffs_dev([0] * 9)
    c = K.commit(srs, d)
    value, proof = K.open(srs, d, Z)
    assert value == 0 and not c.any() and not proof.any()
    assert K.check(srs, c, Z, 0, proof) is True
    assert K.check(srs, c, Z, 1, proof) is False


def test_batched_forms_equal_the_loops(zk, srs):
    import torch

    K = zk.kzg
    n = 300
    p = poly(n, seed=1)
    d = coeffs_dev(p)
    zs = [Z, 0, 1, R - 1, Z]
    values, proofs = K.open_many(srs, d, zs)
    assert proofs.shape == (5, 8)
    for j, z in enumerate(zs):
        v, w = K.open(srs, d, z)
        assert values[j] == v == P.horner(p, z) and np.array_equal(proofs[j], w)
    polys = torch.stack([coeffs_dev(poly(n, seed=s)) for s in range(3)])
    many = K.commit_many(srs, polys)
    for s in range(3):
        assert np.array_equal(many[s], K.commit(srs, polys[s]))


def test_check_many_flags_the_tampered_row(zk, srs):
    K = zk.kzg
    p = poly(64, seed=2)
    d = coeffs_dev(p)
    zs = [(Z + 17 * i) % R for i in range(8)]
    values, proofs = K.open_many(srs, d, zs)
    commitments = np.tile(K.commit(srs, d), (8, 1))
    assert K.check_many(srs, commitments, zs, values, proofs).tolist() == [True] * 8
    values[3] = (values[3] + 1) % R
    ok = K.check_many(srs, commitments, zs, values, proofs)
    assert ok.dtype == bool and ok.tolist() == [i != 3 for i in range(8)]


def test_a_polynomial_longer_than_the_srs_is_refused(zk, srs, geom):
    K = zk.kzg
    d = coeffs_dev([1] * (geom[1] + 2))
    with pytest.raises(ValueError):
        K.commit(srs, d)
    with pytest.raises(ValueError):
        K.open(srs, d, Z)
    with pytest.raises(ValueError):
        K.commit_many(srs, d.reshape(1, -1, 4))
    with pytest.raises(ValueError):
        K.srs_from_accumulator({"tau_g1": srs["g1"], "tau_g2": srs["g1"][:0]}, degree=3)
    with pytest.raises(ValueError):
        K.srs_from_accumulator({"tau_g1": srs["g1"][:4], "tau_g2": srs["g2_one"].repeat(2, 1)}, degree=4)


def test_srs_from_an_accumulator(zk, srs):
    K = zk.kzg
    acc = zk.ceremony.contribute_accumulator(zk.ceremony.new_accumulator(4, "cuda"), TAU, ALPHA, BETA)
    mine = K.srs_from_accumulator(acc)
    assert mine["g1"].data_ptr() == acc["tau_g1"].data_ptr() and mine["g2_tau"].data_ptr() == acc["tau_g2"][1].data_ptr()   # views
    assert K.srs_from_accumulator(acc, degree=20)["g1"].shape[0] == 21
    p = poly(21, seed=3)
    d = coeffs_dev(p)
    c, (value, proof) = K.commit(mine, d), K.open(mine, d, Z)
    assert np.array_equal(c, K.commit(srs, d)) and np.array_equal(c, g1_mul(P.horner(p, TAU)))
    v2, w2 = K.open(srs, d, Z)
    assert value == v2 and np.array_equal(proof, w2)
    assert K.check(mine, c, Z, value, proof) is True
    assert K.check(mine, c, Z, (value + 1) % R, proof) is False
