"""Circuits and witnesses shared by tests/test_r1cs_host.py and tests/test_gpu_r1cs.py, and the big-int model of the sparse Fr product
(Montgomery R = 2^256, r = the group order)."""
import numpy as np

import bn254_model as M

R_ORDER = M.R_ORDER
MONT_R = (1 << 256) % R_ORDER

# the 11-variable circuit of tests/test_circom_host.py
SMALL_JSON = {
    "constraints": [[{"2": "1"}, {"3": "1"}, {"4": "1"}],
                    [{"4": "1", "0": "5"}, {"0": "1"}, {"1": "1"}],
                    [{"10": "7", "9": "3"}, {}, {}]],
    "nPubInputs": 1, "nOutputs": 1, "nVars": 11,
}
SMALL_WITNESS = [1, 11, 2, 3, 6, 0, R_ORDER - 1, 12345678901234567890123456789, 1, 5, 9]


def small_circuit(zk):
    c = zk.circom.circuit_from_json(SMALL_JSON)
    c.witness = list(SMALL_WITNESS)
    return c


def random_circuit(zk, seed=4100, n_constraints=200, num_inputs=5, num_aux=61):
    """A seeded circuit of ~200 constraints with what a term list can hold: empty combinations, a variable repeated within one
    combination, zero coefficients, variable 0 (ONE), a combination of 70 terms; coefficients 1, -1, powers of two, 0 and uniform."""
    rng = np.random.default_rng(seed)
    n_vars = num_inputs + num_aux

    def uniform():
        return int.from_bytes(rng.bytes(40), "little") % R_ORDER

    def coeff():
        k = int(rng.integers(0, 10))
        return (1, 1, 1, R_ORDER - 1, R_ORDER - 1, 1 << int(rng.integers(1, 254)), 2, 0, uniform(), uniform())[k]

    def lc(i, which):
        length = int(rng.choice([0, 1, 1, 2, 2, 3, 3, 5, 9]))
        terms = [(int(rng.integers(0, n_vars)), coeff()) for _ in range(length)]
        if i % 7 == which:
            terms.append((0, coeff()))                     # variable 0
        if i % 11 == which and terms:
            terms.append((terms[0][0], coeff()))           # the same variable twice in one combination
        if i % 13 == which:
            terms.append((int(rng.integers(0, n_vars)), 0))   # a zero coefficient: the variable still counts as dense
        if i == 50 + which:
            terms = [(int(rng.integers(0, n_vars)), coeff()) for _ in range(70)]
        if i == 60 + which:
            terms = []
        return terms

    constraints = [(lc(i, 0), lc(i, 1), lc(i, 2)) for i in range(n_constraints)]
    kinds = rng.integers(0, 10, size=n_vars)
    witness = [1] + [1 if k < 4 else 0 if k < 7 else int(rng.integers(0, 256)) if k == 7 else R_ORDER - 1 if k == 8 else uniform() for k in kinds[1:]]
    return zk.circom.CircomCircuit(num_inputs, num_aux, n_constraints, constraints, witness)


def to_limbs(vals) -> np.ndarray:
    buf = b"".join(int(v).to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


def from_limbs(arr):
    raw = np.ascontiguousarray(arr).view(np.uint64).reshape(-1, 4).tobytes()
    return [int.from_bytes(raw[32 * i:32 * i + 32], "little") for i in range(len(raw) // 32)]


def mont(vals) -> np.ndarray:
    return to_limbs(v % R_ORDER * MONT_R % R_ORDER for v in vals)
