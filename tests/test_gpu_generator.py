"""groth16 generate_parameters on the device (phase2-bn254_amd/generator.py) against parameters worked out with Python big ints -- the
Lagrange coefficients at tau from their closed form, no FFT -- and the oracle's scalar multiplication; and, the trapdoor being known, a
proof over the generated parameters against its closed form in the exponent."""
import numpy as np
import pytest

import bn254_model as M
import fixed_base_cases as FB
import inputs
import oracle_lib as O
import r1cs_cases

pytestmark = pytest.mark.gpu

R = M.R_ORDER
# fixed non-zero toxic waste
ALPHA, BETA, GAMMA, DELTA, TAU = (0x1B7E4D3C2A190807F6E5D4C3B2A1908F7E6D5C4B3A29180706F5E4D3C2B1A09 % R, 0x2468ACE013579BDF02468ACE13579BDF2468ACE013579BDF02468ACE13579BD % R,
                                  0x0123456789ABCDEF0FEDCBA9876543210123456789ABCDEF0FEDCBA98765432 % R, R - 0x5DEECE66D, 0x2F0E1D2C3B4A59687796A5B4C3D2E1F00F1E2D3C4B5A69788796A5B4C3D2E1F % R)


def chain_circuit(zk, steps=4, c=7, x0=3):
    """x_{i+1} = x_i * x_i + c: variable 0 is ONE, 1 the public output x_steps, the aux variables x_0 .. x_{steps-1}; the witness
    satisfies every constraint (checked with big ints)"""
    xs = [x0]
    for _ in range(steps):
        xs.append((xs[-1] * xs[-1] + c) % R)
    var = lambda i: 1 if i == steps else 2 + i  # noqa: E731
    constraints = [([(var(i), 1)], [(var(i), 1)], [(var(i + 1), 1), (0, R - c)]) for i in range(steps)]
    witness = [1, xs[steps]] + xs[:steps]
    for a, b, cc in constraints:
        ev = lambda lc: sum(k * witness[v] for v, k in lc) % R  # noqa: E731
        assert ev(a) * ev(b) % R == ev(cc)
    return zk.circom.CircomCircuit(2, steps, steps, constraints, witness)


def qap_at_tau(zk, circuit):
    """(cs, m, A_v, B_v, C_v at tau for every variable, inputs first) from L_j(tau) = (tau^m - 1) / m * omega^j / (tau - omega^j)"""
    cs = zk.circom.assemble(circuit)
    exp = zk.circom.domain_exponent(cs.num_constraints)
    m = 1 << exp
    omega = M.domain_omega(exp)
    front = (pow(TAU, m, R) - 1) * pow(m, -1, R) % R
    lag, w = [], 1
    for _ in range(m):
        lag.append(front * w % R * pow(TAU - w, -1, R) % R)
        w = w * omega % R
    ev = lambda rows: [sum(c * lag[j] for c, j in row) % R for row in rows]  # noqa: E731
    return cs, m, ev(cs.at_inputs + cs.at_aux), ev(cs.bt_inputs + cs.bt_aux), ev(cs.ct_inputs + cs.ct_aux)


def expected_parameters(zk, circuit):
    cs, m, A, B, Cc = qap_at_tau(zk, circuit)
    g1, g2 = inputs.G1_GEN_RAW, inputs.G2_GEN_RAW
    mul1 = lambda ks: O.G1.mul_many_affine(g1, FB.limbs(ks)) if len(ks) else np.zeros((0, 8), np.uint64)  # noqa: E731
    mul2 = lambda ks: O.G2.mul_many_affine(g2, FB.limbs(ks)) if len(ks) else np.zeros((0, 16), np.uint64)  # noqa: E731
    t = (pow(TAU, m, R) - 1) % R
    dinv, ginv = pow(DELTA, -1, R), pow(GAMMA, -1, R)
    ext = [(BETA * a + ALPHA * b + c) * (ginv if v < cs.num_inputs else dinv) % R for v, (a, b, c) in enumerate(zip(A, B, Cc))]
    return {"h": mul1([pow(TAU, i, R) * t % R * dinv % R for i in range(m - 1)]),
            "l": mul1(ext[cs.num_inputs:]), "ic": mul1(ext[:cs.num_inputs]),
            "a": mul1([a for a in A if a]), "b_g1": mul1([b for b in B if b]), "b_g2": mul2([b for b in B if b]),
            "alpha_g1": mul1([ALPHA]), "beta_g1": mul1([BETA]), "delta_g1": mul1([DELTA]),
            "beta_g2": mul2([BETA]), "gamma_g2": mul2([GAMMA]), "delta_g2": mul2([DELTA])}


def generate(zk, circuit, gamma=GAMMA, delta=DELTA):
    return zk.generator.generate_parameters(circuit, inputs.G1_GEN_RAW, inputs.G2_GEN_RAW, ALPHA, BETA, gamma, delta, TAU, "cuda")


def host(t):
    return t.cpu().numpy().view(np.uint64)


@pytest.mark.parametrize("which", ["small", "random", "chain"])
def test_parameters_match_big_ints(zk, worker, which):
    circuit = {"small": r1cs_cases.small_circuit, "random": lambda z: r1cs_cases.random_circuit(z, n_constraints=200), "chain": chain_circuit}[which](zk)
    want = expected_parameters(zk, circuit)
    if which == "random":
        assert want["h"].shape[0] == 255 and want["ic"].shape[0] + want["l"].shape[0] == 66
    if which == "small":
        # four of its aux variables are in no constraint: the reference returns UnconstrainedVariable for it (generator.rs:477-483), and so
        # does generate_parameters; every vector is compared all the same, on what is computed before that test
        assert int((~want["l"].any(axis=1)).sum()) == 4
        with pytest.raises(zk.SynthesisError) as e:
            generate(zk, circuit)
        assert e.value.kind == zk.SynthesisError.UNCONSTRAINED_VARIABLE
        p = zk.generator._queries(circuit, inputs.G1_GEN_RAW, inputs.G2_GEN_RAW, ALPHA, BETA, GAMMA, DELTA, TAU, "cuda")
    else:
        p = generate(zk, circuit)
    for k in ("h", "l", "a", "b_g1", "b_g2"):
        got = host(p[k])
        assert got.shape == want[k].shape and np.array_equal(got, want[k]), (which, k)
    assert np.array_equal(host(p["vk"]["ic"]), want["ic"])
    for k in ("alpha_g1", "beta_g1", "beta_g2", "gamma_g2", "delta_g1", "delta_g2"):
        assert np.array_equal(host(p["vk"][k]).reshape(-1), want[k].reshape(-1)), (which, k)


def test_proof_in_the_exponent(zk, worker):
    """with the trapdoor known a proof needs no pairing check: A, B and C are fixed multiples of the generators"""
    circuit = chain_circuit(zk)
    cs, m, A, B, Cc = qap_at_tau(zk, circuit)
    w = circuit.witness
    r, s = 0x3C4B5A69788796A5B4C3D2E1F00F1E2D % R, 0x1F2E3D4C5B6A79880796A5B4C3D2E1F0 % R
    swa, swb, swc = (sum(wv * x for wv, x in zip(w, X)) % R for X in (A, B, Cc))
    a_exp = (ALPHA + swa + r * DELTA) % R
    b_exp = (BETA + swb + s * DELTA) % R
    aux = sum(w[v] * (BETA * A[v] + ALPHA * B[v] + Cc[v]) for v in range(cs.num_inputs, len(w))) % R
    c_exp = ((aux + swa * swb - swc) * pow(DELTA, -1, R) + s * a_exp + r * b_exp - r * s * DELTA) % R
    pa, pb, pc = zk.circom.prove(worker, circuit, generate(zk, circuit), r, s)
    assert np.array_equal(np.asarray(pa, dtype=np.uint64).reshape(-1), O.G1.mul_many_affine(inputs.G1_GEN_RAW, FB.limbs([a_exp]))[0])
    assert np.array_equal(np.asarray(pb, dtype=np.uint64).reshape(-1), O.G2.mul_many_affine(inputs.G2_GEN_RAW, FB.limbs([b_exp]))[0])
    assert np.array_equal(np.asarray(pc, dtype=np.uint64).reshape(-1), O.G1.mul_many_affine(inputs.G1_GEN_RAW, FB.limbs([c_exp]))[0])


def test_errors(zk, worker):
    circuit = chain_circuit(zk)
    for gamma, delta in ((0, DELTA), (GAMMA, 0), (R, DELTA)):
        with pytest.raises(zk.SynthesisError) as e:
            generate(zk, circuit, gamma=gamma, delta=delta)
        assert e.value.kind == zk.SynthesisError.UNEXPECTED_IDENTITY
    loose = chain_circuit(zk)
    loose.num_aux += 1                                    # one more aux variable, in no constraint
    loose.witness = loose.witness + [5]
    with pytest.raises(zk.SynthesisError) as e:
        generate(zk, loose)
    assert e.value.kind == zk.SynthesisError.UNCONSTRAINED_VARIABLE
