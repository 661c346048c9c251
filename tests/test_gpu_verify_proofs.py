"""Many Groth16 proofs against one verifying key on the device (phase2-bn254_amd/pairing.py: prepare_verifying_key_dev, input_accumulators,
verify_proofs_dev, batch_pairs, verify_proofs_batch, read_proofs / write_proofs).  The key has KNOWN logarithms, so proofs are simulated
from scalars: ic_j = u_j G1, A = a G1, B = b G2, C = ((a b - alpha beta - gamma (u_0 + sum_j x_j u_j)) / delta) G1.  Expectations come
from the oracle and from verify_proofs (the unchanged baseline), never from the code under test."""
import numpy as np
import pytest

import bn254_model as M
import fixed_base_cases as FB
import fixed_bases_cases as FBS
import inputs
import oracle_lib as O
from test_gpu_pairing import ALPHA, BETA, DELTA, GAMMA, TAU, batch_mul, chain_circuit, dev, host

pytestmark = pytest.mark.gpu

R = M.R_ORDER
ELLS = (0, 1, 5, 40)
SIZES = (1, 2, 33, 257)
N_MAX = max(SIZES)
KEY = bytes(range(32))


class Sim:
    """one key with l public inputs and N_MAX honest proofs over it, as logarithms and as device records"""

    def __init__(self, zk, ell):
        self.ell = ell
        self.u = FB.ints(inputs.random_scalars(ell + 1, seed=9500 + ell))
        self.x = [FB.ints(row) for row in inputs.random_scalars(N_MAX * ell, seed=9510 + ell).reshape(N_MAX, ell, 4)] if ell else [[] for _ in range(N_MAX)]
        self.a = FB.ints(inputs.random_scalars(N_MAX, seed=9520 + ell))
        self.b = FB.ints(inputs.random_scalars(N_MAX, seed=9530 + ell))
        self.c = [self.c_log(i, self.x[i]) for i in range(N_MAX)]
        g1 = host(batch_mul(zk, 1, [ALPHA] + self.u))
        g2 = host(batch_mul(zk, 2, [BETA, GAMMA, DELTA]))
        self.vk = {"alpha_g1": g1[0].copy(), "beta_g2": g2[0].copy(), "gamma_g2": g2[1].copy(), "delta_g2": g2[2].copy(), "ic": np.ascontiguousarray(g1[1:])}
        self.pvk = zk.pairing.prepare_verifying_key_dev(self.vk)
        self.A, self.B, self.C = batch_mul(zk, 1, self.a), batch_mul(zk, 2, self.b), batch_mul(zk, 1, self.c)

    def c_log(self, i, x):
        acc = (self.u[0] + sum(xj * uj for xj, uj in zip(x, self.u[1:]))) % R
        return (self.a[i] * self.b[i] - ALPHA * BETA - GAMMA * acc) * pow(DELTA, -1, R) % R

    def proofs(self, n):
        return self.A[:n].contiguous(), self.B[:n].contiguous(), self.C[:n].contiguous()

    def inputs(self, n):
        return np.ascontiguousarray(np.array([[M.to_limbs(v) for v in row] for row in self.x[:n]], dtype=np.uint64).reshape(n, self.ell, 4))


_sims = {}


@pytest.fixture
def sim(zk, worker):
    def get(ell):
        if ell not in _sims:
            _sims[ell] = Sim(zk, ell)
        return _sims[ell]

    return get


@pytest.mark.parametrize("ell", ELLS)
def test_input_accumulators_match_the_oracle(zk, sim, ell):
    s = sim(ell)
    want = FBS.want_lincomb(s.vk["ic"][1:], s.vk["ic"][0], s.inputs(N_MAX))
    for n in SIZES:
        for form in (s.x[:n], s.inputs(n), dev(s.inputs(n))):                     # nested lists, numpy, device tensor
            got = host(zk.pairing.input_accumulators(s.pvk, form))
            assert got.shape == (n, 8) and np.array_equal(got, want[:n]), (ell, n)
    if ell == 0:
        assert np.array_equal(want, np.tile(s.vk["ic"][0], (N_MAX, 1)))


@pytest.mark.parametrize("ell", ELLS)
def test_honest_and_tampered_batches(zk, sim, ell):
    import torch

    s = sim(ell)
    for n in SIZES:
        a, b, c = s.proofs(n)
        x = s.inputs(n)
        assert zk.pairing.verify_proofs_dev(s.pvk, (a, b, c), x).tolist() == [True] * n, (ell, n)
        assert zk.pairing.verify_proofs_batch(s.pvk, (a, b, c), x, key=KEY) is True, (ell, n)
        for bad in sorted({0, n // 2, n - 1}):
            kinds = ["two_c", "swap"] + (["input"] if ell else [])
            for kind in kinds:
                a2, c2, x2 = a.clone(), c.clone(), x.copy()
                if kind == "two_c":
                    c2[bad] = batch_mul(zk, 1, [2 * s.c[bad]])[0]
                elif kind == "swap":
                    a2[bad], c2[bad] = c[bad], a[bad]
                else:
                    x2[bad, 0] = M.to_limbs((s.x[bad][0] + 1) % R)
                want = [i != bad for i in range(n)]
                assert zk.pairing.verify_proofs_dev(s.pvk, (a2, b, c2), x2).tolist() == want, (ell, n, bad, kind)
                assert zk.pairing.verify_proofs_batch(s.pvk, (a2, b, c2), x2, key=KEY) is False, (ell, n, bad, kind)
    torch.cuda.synchronize()


def test_list_form_and_the_baseline_agree(zk, sim):
    """the same 33 simulated proofs through verify_proofs (the unchanged baseline) and verify_proofs_dev in its list form"""
    s = sim(5)
    n = 33
    a, b, c = (host(t) for t in s.proofs(n))
    proofs = [(a[i], b[i], c[i]) for i in range(n)]
    pubs = [list(row) for row in s.x[:n]]
    proofs[0], proofs[32] = (a[0], b[0], a[0]), (c[32], b[32], a[32])
    pubs[16] = [pubs[16][0] + 1] + pubs[16][1:]
    proofs[7] = (np.zeros(8, np.uint64), b[7], c[7])                            # an all-zero record contributes one
    base = zk.pairing.verify_proofs(s.pvk, proofs, pubs)
    assert base.tolist() == [i not in (0, 7, 16, 32) for i in range(n)]
    assert zk.pairing.verify_proofs_dev(s.pvk, proofs, pubs).tolist() == base.tolist()


def test_real_proofs_and_the_malformed_key(zk, worker):
    """the 33-proof list of test_gpu_pairing.py::test_verify_proof: this library's generator and prover"""
    import torch

    circuit = chain_circuit(zk)
    params = zk.generator.generate_parameters(circuit, inputs.G1_GEN_RAW, inputs.G2_GEN_RAW, ALPHA, BETA, GAMMA, DELTA, TAU, "cuda")
    r, s = 0x3C4B5A69788796A5B4C3D2E1F00F1E2D % R, 0x1F2E3D4C5B6A79880796A5B4C3D2E1F0 % R
    a, b, c = (np.asarray(p, dtype=np.uint64).reshape(-1) for p in zk.circom.prove(worker, circuit, params, r, s))
    pvk = zk.pairing.prepare_verifying_key_dev(params["vk"])
    public = [circuit.witness[1]]
    two_c = zk.prover._to_affine(zk.prover._mul(c, 2))
    proofs, pubs = [(a, b, c)] * 33, [public] * 33
    proofs[0], proofs[32] = (a, b, two_c), (c, b, a)
    pubs[16] = [public[0] + 1]
    want = zk.pairing.verify_proofs(pvk, proofs, pubs)
    assert want.tolist() == [i not in (0, 16, 32) for i in range(33)]
    assert zk.pairing.verify_proofs_dev(pvk, proofs, pubs).tolist() == want.tolist()
    assert zk.pairing.verify_proofs_batch(pvk, proofs, pubs, key=KEY) is False
    assert zk.pairing.verify_proofs_batch(pvk, [(a, b, c)] * 33, [public] * 33, key=KEY) is True
    # len(public_inputs) + 1 != len(ic): raised before any device work -- the proofs here are not even tensors
    for fn in (zk.pairing.verify_proofs_dev, zk.pairing.verify_proofs_batch):
        with pytest.raises(zk.SynthesisError) as e:
            fn(pvk, [(None, None, None)], [public + [1]])
        assert e.value.kind == zk.SynthesisError.MALFORMED_VERIFYING_KEY
    with pytest.raises(zk.SynthesisError):
        zk.pairing.input_accumulators(pvk, torch.zeros((4, 2, 4), dtype=torch.int64, device="cuda"))
    with pytest.raises(zk.SynthesisError):
        zk.pairing.input_accumulators(pvk, np.zeros((4, 0, 4), np.uint64))


def _g1_sum(records):
    acc = O.G1.from_affine(np.zeros(8, np.uint64))
    for rec in records:
        if rec.any():
            acc = O.G1.add(acc, O.G1.from_affine(rec))
    return O.G1.to_affine(acc)


@pytest.mark.parametrize("n,ell", [(5, 3), (33, 1)])
def test_batch_pairs_match_the_oracle(zk, sim, n, ell):
    s = Sim(zk, ell) if ell not in ELLS else sim(ell)
    a, b, c = s.proofs(n)
    g1, g2 = zk.pairing.batch_pairs(s.pvk, (a, b, c), s.inputs(n), KEY)
    assert tuple(g1.shape) == (n + 3, 8) and tuple(g2.shape) == (n + 3, 16)
    r = zk.ceremony.fr_random_host(n, KEY, 0)
    ri = FB.ints(r)
    ha, hc = host(a), host(c)
    want_ra = np.stack([O.G1.mul_many_affine(np.ascontiguousarray(ha[i]), r[i:i + 1])[0] for i in range(n)])
    sums = [sum(ri) % R] + [sum(ri[i] * s.x[i][j] for i in range(n)) % R for j in range(ell)]
    t = FBS.want_lincomb(s.vk["ic"], None, FBS.scalar_rows([sums]))[0]
    sum_c = _g1_sum([O.G1.mul_many_affine(np.ascontiguousarray(hc[i]), r[i:i + 1])[0] for i in range(n)])
    neg_alpha = O.G1.mul_many_affine(s.vk["alpha_g1"], FB.limbs([(R - sums[0]) % R]))[0]
    got1, got2 = host(g1), host(g2)
    assert np.array_equal(got1[:n], want_ra)
    assert np.array_equal(got1[n], t) and np.array_equal(got1[n + 1], sum_c) and np.array_equal(got1[n + 2], neg_alpha)
    assert np.array_equal(got2[:n], host(b))
    assert np.array_equal(got2[n], s.pvk["neg_gamma_g2"]) and np.array_equal(got2[n + 1], s.pvk["neg_delta_g2"]) and np.array_equal(got2[n + 2], s.vk["beta_g2"])


def _product_is_one(zk, g1, g2):
    import torch

    ptr = torch.tensor([0, int(g1.shape[0])], dtype=torch.int32, device="cuda")
    return bool(zk.pairing.gt_eq(zk.pairing.pairing_product(g1, g2, ptr))[0].item())


def test_errors_that_cancel_without_weights(zk, sim):
    """C_0 + D and C_1 - D: with every weight one the product IS one; with random weights it is not, whatever the key"""
    import torch

    s = sim(5)
    n = 2
    a, b, c = s.proofs(n)
    d = 0x5A5A5A5A5A5A5A5A1234 % R
    c = batch_mul(zk, 1, [(s.c[0] + d) % R, (s.c[1] - d) % R])
    x = s.inputs(n)
    ones = dev(FB.limbs([1, 1]))
    assert _product_is_one(zk, *zk.pairing.batch_pairs(s.pvk, (a, b, c), x, KEY, coefficients=ones))
    for key in (KEY, bytes(32), bytes(reversed(range(32)))):
        assert not _product_is_one(zk, *zk.pairing.batch_pairs(s.pvk, (a, b, c), x, key))
        assert zk.pairing.verify_proofs_batch(s.pvk, (a, b, c), x, key=key) is False
    assert zk.pairing.verify_proofs_dev(s.pvk, (a, b, c), x).tolist() == [False, False]
    assert zk.pairing.verify_proofs_batch(s.pvk, s.proofs(n), x) is True                       # key=None: os.urandom
    torch.cuda.synchronize()


def test_rejections(zk, sim):
    from test_g2_subgroup import _twist_point

    s = sim(1)
    n = 33
    x = s.inputs(n)
    for which in range(3):
        abc = [t.clone() for t in s.proofs(n)]
        abc[which][17] = 0
        assert zk.pairing.verify_proofs_batch(s.pvk, tuple(abc), x, key=KEY) is False, which
    a, b, c = s.proofs(n)
    b = b.clone()
    b[32] = dev(_twist_point(77))
    assert zk.pairing.verify_proofs_batch(s.pvk, (a, b, c), x, key=KEY) is False
    assert isinstance(zk.pairing.verify_proofs_batch(s.pvk, (a, b, c), x, key=KEY, check_g2_subgroup=False), bool)
    assert zk.pairing.verify_proofs_batch(s.pvk, s.proofs(n), x, key=KEY, check_g2_subgroup=False) is True


def test_read_and_write_proofs(zk, sim):
    import torch

    s = sim(1)
    n = 33
    a, b, c = s.proofs(n)
    data = zk.pairing.write_proofs(a, b, c)
    assert data.dtype == torch.uint8 and tuple(data.shape) == (128 * n,)
    first = torch.cat([zk.ceremony.encode_points(a[:1], True), zk.ceremony.encode_points(b[:1], True), zk.ceremony.encode_points(c[:1], True)], dim=1).reshape(-1)
    assert torch.equal(data[:128], first)
    a2, b2, c2 = zk.pairing.read_proofs(data)
    assert torch.equal(a2, a) and torch.equal(b2, b) and torch.equal(c2, c)
    bad = data.clone()
    bad[17 * 128 + 96 + 1:17 * 128 + 128] = 0xFF                                  # C of proof 17: x >= q
    bad[17 * 128 + 96] |= 0x3F
    with pytest.raises(zk.ceremony.GroupDecodingError) as e:
        zk.pairing.read_proofs(bad)
    assert e.value.index == 17
    inf = data.clone()
    inf[5 * 128:5 * 128 + 32] = 0
    inf[5 * 128] = 0x40                                                          # A of proof 5: the infinity encoding
    with pytest.raises(zk.ceremony.DeserializationError):
        zk.pairing.read_proofs(inf)
