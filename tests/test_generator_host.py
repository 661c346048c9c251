"""The host half of generator.py (no GPU): the per-variable term lists as one CSR matrix with host-scaled coefficient tables, evaluated
with big ints on the Lagrange coefficients at tau, give A_v, B_v and (beta A_v + alpha B_v + C_v) * inv of every variable."""
import pytest

import bn254_model as M
import r1cs_cases
import test_gpu_generator as T

R = M.R_ORDER


@pytest.mark.parametrize("which", ["small", "random", "chain"])
def test_qap_matrix_rows_are_the_polynomials_at_tau(zk, which):
    circuit = {"small": r1cs_cases.small_circuit, "random": lambda z: r1cs_cases.random_circuit(z, n_constraints=200), "chain": T.chain_circuit}[which](zk)
    cs, m, A, B, Cc = T.qap_at_tau(zk, circuit)
    ginv, dinv = pow(T.GAMMA, -1, R), pow(T.DELTA, -1, R)
    q = zk.generator._qap_matrix(cs, T.ALPHA, T.BETA, ginv, dinv)
    n_vars = q["n_vars"]
    assert n_vars == len(A) == cs.num_inputs + cs.num_aux and q["row_ptr"].shape[0] == 3 * n_vars + 1
    assert int(q["row_ptr"][0]) == 0 and int(q["row_ptr"][-1]) == q["col"].shape[0] == q["coeff_id"].shape[0]
    assert q["col"].size == 0 or int(q["col"].max()) < m
    omega = M.domain_omega(zk.circom.domain_exponent(cs.num_constraints))
    front = (pow(T.TAU, m, R) - 1) * pow(m, -1, R) % R
    lag = [front * pow(omega, j, R) % R * pow(T.TAU - pow(omega, j, R), -1, R) % R for j in range(m)]
    coeffs = [M.from_mont(v, R) for v in r1cs_cases.from_limbs(q["coeffs"])]
    assert len(set(coeffs)) == len(coeffs)                 # a table of DISTINCT values
    rows = [sum(coeffs[int(q["coeff_id"][t])] * lag[int(q["col"][t])] for t in range(int(q["row_ptr"][r]), int(q["row_ptr"][r + 1]))) % R
            for r in range(3 * n_vars)]
    ext = [(T.BETA * a + T.ALPHA * b + c) * (ginv if v < cs.num_inputs else dinv) % R for v, (a, b, c) in enumerate(zip(A, B, Cc))]
    assert rows[:n_vars] == A and rows[n_vars:2 * n_vars] == B and rows[2 * n_vars:] == ext


def test_zero_gamma_or_delta_is_refused_before_any_device_work(zk):
    import inputs

    for gamma, delta in ((0, 5), (5, 0), (R, 5)):
        with pytest.raises(zk.SynthesisError) as e:
            zk.generator.generate_parameters(T.chain_circuit(zk), inputs.G1_GEN_RAW, inputs.G2_GEN_RAW, 2, 3, gamma, delta, 7, "cuda")
        assert e.value.kind == zk.SynthesisError.UNEXPECTED_IDENTITY
