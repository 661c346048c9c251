"""Shared by the prepare_phase2 tests (not a test module): the shifted-difference cases as lists of small multiples of the G1 generator with
their big-int expectation (tests/bn254_model.py), and the closed forms of a phase1radix2m file from known secrets."""
import functools

import numpy as np

import bn254_model as M

G1 = (1, 2)
K = 16                                                             # MI355ZK_SHIFTED_DIFFERENCE_K; the tests assert that it is the library's
SPAN = 48                                                          # |multiple| of every case stays below this, so |difference| < 2 * SPAN


@functools.lru_cache(maxsize=None)
def _table():
    """k * G for 0 <= k < 2 * SPAN by repeated addition (None: infinity)"""
    out = [None]
    for _ in range(2 * SPAN - 1):
        out.append(M.ec_add(M.FQ_OPS, out[-1], G1))
    return out


def small_multiple(k: int):
    """k * G, |k| < 2 * SPAN, as an affine big-int pair or None"""
    p = _table()[abs(k)]
    return M.ec_neg(M.FQ_OPS, p) if k < 0 else p


def raw(multiples) -> np.ndarray:
    """(n, 8) u64 raw affine records of the multiples (0: the all-zero record)"""
    return np.array([M.g1_affine_to_raw(small_multiple(k)) for k in multiples], dtype=np.uint64).reshape(len(multiples), 8)


def expected(multiples, shift: int, n_out: int) -> np.ndarray:
    """out[i] = (multiples[i + shift] - multiples[i]) * G, from the integers"""
    return raw([multiples[i + shift] - multiples[i] for i in range(n_out)])


def mixed(n: int, seed: int = 0):
    """n multiples in a fixed pseudo-random order, infinities and repeats among them"""
    state, out = 12345 + seed, []
    for _ in range(n):
        state = (state * 1103515245 + 12345) % (1 << 31)
        out.append((state >> 8) % 23 - 11)
    return out


def _pairs(a, b):
    """in[i] = a[i], in[i + len(a)] = b[i]: the operands of one group at shift = n_out = len(a)"""
    assert len(a) == len(b)
    return list(a) + list(b), len(a), len(a)


# (name, multiples, shift, n_out): every case of the lane routine inside ONE shared inversion, then groups that are all one exceptional case
_A = [3, 5, 4, 0, 6, 0, 7, 9, 9, -2, 0, 8, 1, 0, 11, 2]
_B = [7, 5, -4, 9, 0, 0, 1, 9, -9, 2, 3, 0, 1, 0, -11, 10]         # generic, equal, opposite, left inf, right inf, both inf, ...
CASES = [
    ("every case in one group",) + _pairs(_A, _B),
    ("every case in one group, shift 1", [1, 3, 3, -3, 0, 5, 0, 0, 2, 2, -2, 7, 0, 4, -4, -4, 9], 1, K),
    ("all equal", [5] * (K + 1), 1, K),
    ("all opposite", [4 if i % 2 == 0 else -4 for i in range(K + 1)], 1, K),
    ("all both infinite", [0] * (2 * K), K, K),
    ("all left infinite",) + _pairs([0] * K, list(range(1, K + 1))),
    ("all right infinite",) + _pairs(list(range(1, K + 1)), [0] * K),
    ("one chord among infinities",) + _pairs([0] * 7 + [2] + [0] * 8, [0] * 7 + [9] + [0] * 8),
]
for _n_out in (1, K - 1, K, K + 1, 2 * K + 1):
    for _shift in (1, _n_out, _n_out + 3):
        CASES.append((f"n_out {_n_out} shift {_shift}", mixed(_shift + _n_out + 2, _n_out * 7 + _shift), _shift, _n_out))
CASE_IDS = [c[0] for c in CASES]


# ---------------------------------------------------------------- closed forms of a radix file
def lagrange_at(tau: int, m: int):
    """L_j(tau), j < m, over the size-m domain of Fr: the inverse DFT of the powers of tau, (1 / m) sum_i tau^i omega^(-i j)"""
    r = M.R_ORDER
    omega_inv = pow(M.domain_omega(m.bit_length() - 1), -1, r)
    m_inv = pow(m, -1, r)
    powers = [pow(tau, i, r) for i in range(m)]
    return [m_inv * sum(powers[i] * pow(omega_inv, i * j, r) for i in range(m)) % r for j in range(m)]


def radix_scalars(tau: int, alpha: int, beta: int, m: int):
    """{section: [scalar of every record]} of phase1radix2m{log2 m} for an accumulator with these secrets (each record is scalar * generator)"""
    r = M.R_ORDER
    lag = lagrange_at(tau, m)
    return {"alpha_g1": [alpha % r], "beta_g1": [beta % r], "beta_g2": [beta % r], "coeffs_g1": lag, "coeffs_g2": lag,
            "alpha_coeffs_g1": [alpha * v % r for v in lag], "beta_coeffs_g1": [beta * v % r for v in lag],
            "h": [(pow(tau, i + m, r) - pow(tau, i, r)) % r for i in range(m - 1)]}
