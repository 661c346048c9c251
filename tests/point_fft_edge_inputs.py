"""Structured inputs for the curve-point FFTs (csrc/point_fft.hip, point_fft_g2.hip) with their expectations.

TEST INFRASTRUCTURE, plain Python, no GPU.  One table that both legs import: tests/test_point_fft_edges_host.py (the table, its closed forms
and what each family is there for, against the CPU oracle) and tests/test_gpu_point_fft_edges.py (the same vectors through
mi355zk_bn254_g{1,2}_point_fft_dev).

The existing parity tests feed the transforms distinct points, so every addition of every butterfly is the generic one.  The vectors here
are multiples s_i * P of ONE fixed random point P of order r, chosen so that butterflies meet equal operands (u + w t is a doubling, u - w t
infinity), opposite ones, an infinite u or t, whole stages of infinities, and outputs that are infinity in whole normalisation groups.
A vector knows its scalars s_i (None where it is not a multiple table), so

  * its input records come from the oracle's scalar multiplication of P  (oracle: mul_many_affine), and
  * its expectation, where the family has a closed form, is a handful of (index, scalar) pairs turned into records by the big-int model of
    tests/bn254_model.py alone (affine group law on Python ints; nothing of oracle/ is involved) -- `Vector.expect(op)`.

`butterflies(...)` replays the kernels' network (bit-reversed load, stage s pairs i0 = (b >> s << s + 1) + j with i0 + 2^s under the twiddle
omega^(j 2^(log_n - 1 - s))) on the SCALARS, which is how the host test states what a family makes the butterflies meet.

n = 2^log_n, omega = bn254_model.domain_omega(log_n) throughout; fft is X_j = sum_i omega^(ij) v_i, ifft its inverse (domain.rs:154-173).
"""
from __future__ import annotations

import functools

import numpy as np

import bn254_model as M
import inputs

R = M.R_ORDER
LOG_N = {1: tuple(range(1, 10)), 2: tuple(range(1, 8))}    # every size of the closed-form families, per group
LOG_N_ORACLE_ONLY = {1: (3, 6, 9), 2: (3, 5, 7)}           # mirrored_progression, half_infinite_*: the oracle decides
NORMALISE_GROUP = {1: 16, 2: 8}                            # records per inversion of batch_normalize_kernel (api.hip)
BASE_SEED = {1: 0x9F17, 2: 0x9F27}
ORACLE_ONLY = ("mirrored_progression", "half_infinite_low", "half_infinite_high")


# ------------------------------------------------------------------------------------------------ the point P and its multiples
def _ops(group):
    return M.FQ_OPS if group == 1 else M.FQ2_OPS


def _to_raw(group, p):
    return M.g1_affine_to_raw(p) if group == 1 else M.g2_affine_to_raw(p)


def _from_raw(group, rec):
    return M.g1_affine_from_raw(rec) if group == 1 else M.g2_affine_from_raw(rec)


@functools.lru_cache(maxsize=None)
def base_scalar(group: int) -> int:
    """P = base_scalar * generator: uniform below r, fixed by BASE_SEED"""
    return M.from_limbs(inputs.random_scalars(1, BASE_SEED[group])[0])


@functools.lru_cache(maxsize=None)
def base_point_raw(group: int) -> np.ndarray:
    """P as a raw affine record, from the oracle's mul_many_affine of the generator (a multiple of the generator: in the order-r subgroup of G2)"""
    import oracle_lib as O

    G = O.G1 if group == 1 else O.G2
    gen = inputs.G1_GEN_RAW if group == 1 else inputs.G2_GEN_RAW
    p = G.mul_many_affine(gen, np.array([M.to_limbs(base_scalar(group))], dtype=np.uint64))[0]
    assert p.any()
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _fixed_base_table(group: int):
    """tab[i][d] = d * 16^i * P (affine big ints, None = infinity), i < 64, d < 16"""
    F = _ops(group)
    tab, b = [], _from_raw(group, base_point_raw(group))
    for _ in range(64):
        row = [None, b]
        for _ in range(2, 16):
            row.append(M.ec_add(F, row[-1], b))
        tab.append(row)
        b = M.ec_add(F, row[15], b)
    return tab


@functools.lru_cache(maxsize=None)
def multiple_raw(group: int, s: int) -> tuple:
    """the raw affine record of s * P (s mod r) by the big-int model: 64 affine additions over the fixed-base table"""
    F, tab, acc = _ops(group), _fixed_base_table(group), None
    s %= R
    for i in range(64):
        acc = M.ec_add(F, acc, tab[i][(s >> (4 * i)) & 15])
    return tuple(_to_raw(group, acc))


def records_of(group: int, sparse: dict, n: int) -> np.ndarray:
    """{index: scalar} -> (n, 8 * group) records: s * P at the named indices (big-int model), infinity (all zero) everywhere else"""
    out = np.zeros((n, 8 * group), dtype=np.uint64)
    for i, s in sparse.items():
        assert 0 <= i < n
        out[i] = multiple_raw(group, s)
    return out


def negate_records(group: int, recs: np.ndarray) -> np.ndarray:
    """-v for raw affine records (infinity stays all zero)"""
    F = _ops(group)
    return np.array([_to_raw(group, M.ec_neg(F, _from_raw(group, r))) for r in recs], dtype=np.uint64).reshape(recs.shape)


# ------------------------------------------------------------------------------------------------ the network on scalars
def bit_reverse(i: int, log_n: int) -> int:
    return int(format(i, "0%db" % log_n)[::-1], 2) if log_n else 0


def butterflies(scalars, log_n: int, inverse: bool):
    """Replays the stage loop of pfft_stage_kernel on scalars mod r.  Returns (trace, out): trace = [(stage, j, u, w, t)] for every butterfly
    (a[i0], a[i1] = u + w t, u - w t), out = the final array (ifft: times 1/n, the kernel's mode-1 pass)."""
    n = 1 << log_n
    w_n = M.domain_omega(log_n)
    if inverse:
        w_n = pow(w_n, -1, R)
    a = [0] * n
    for i, s in enumerate(scalars):
        a[bit_reverse(i, log_n)] = s % R
    trace = []
    for s in range(log_n):
        m = 1 << s
        for b in range(n // 2):
            j = b & (m - 1)
            i0 = ((b >> s) << (s + 1)) + j
            i1 = i0 + m
            w = pow(w_n, j << (log_n - 1 - s), R)
            u, t = a[i0], a[i1]
            trace.append((s, j, u, w, t))
            a[i0], a[i1] = (u + w * t) % R, (u - w * t) % R
    if inverse:
        ninv = pow(n, -1, R)
        a = [v * ninv % R for v in a]
    return trace, a


# ------------------------------------------------------------------------------------------------ the vectors
class Vector:
    """name, group, log_n;  scalars: the s_i (ints mod r) with v_i = s_i P, or None;  points: (n, 8 * group) raw affine records (read-only);
    closed[op]: {index: scalar} of the non-infinite outputs, or None when only the oracle decides"""

    def __init__(self, name, group, log_n, scalars, points, closed):
        self.name, self.group, self.log_n, self.n = name, group, log_n, 1 << log_n
        self.scalars, self.closed = scalars, closed
        points = np.ascontiguousarray(points, dtype=np.uint64)
        assert points.shape == (self.n, 8 * group)
        points.setflags(write=False)
        self.points = points

    def expect(self, op: str):
        """the closed-form output records of `op` ("fft" / "ifft"), or None"""
        if self.closed is None:
            return None
        return records_of(self.group, self.closed[op], self.n)

    def __repr__(self):
        return "Vector(%s, G%d, 2^%d)" % (self.name, self.group, self.log_n)


def _delta_positions(n):
    return {"delta_0": 0, "delta_1": 1, "delta_half": n // 2, "delta_last": n - 1}


def _frequencies(n):
    return {"frequency_1": 1 % n, "frequency_5": 5 % n, "frequency_half": n // 2, "frequency_last": n - 1}


def _distinct(named: dict) -> dict:
    """drops a name whose value an earlier name already has (n = 2 and 4 fold the positions together)"""
    out, seen = {}, set()
    for k, v in named.items():
        if v not in seen:
            seen.add(v)
            out[k] = v
    return out


def closed_form_names(log_n: int) -> list:
    n = 1 << log_n
    return ["constant", "all_infinity"] + list(_distinct(_delta_positions(n))) + list(_distinct(_frequencies(n))) + ["two_frequencies"]


def names(group: int, log_n: int) -> list:
    """every vector name at this size: the closed-form families at every size of LOG_N, the oracle-only ones at LOG_N_ORACLE_ONLY"""
    assert log_n in LOG_N[group]
    return closed_form_names(log_n) + (list(ORACLE_ONLY) if log_n in LOG_N_ORACLE_ONLY[group] else [])


def _multiples_by_oracle(group, scalars):
    """s_i * P through the oracle's scalar multiplication; s_i == 0 -> the all-zero record"""
    import oracle_lib as O

    G = O.G1 if group == 1 else O.G2
    ks = np.array([M.to_limbs(s % R) for s in scalars], dtype=np.uint64)
    pts = G.mul_many_affine(base_point_raw(group), ks)
    for i, s in enumerate(scalars):
        assert pts[i].any() == (s % R != 0), i
    return pts


@functools.lru_cache(maxsize=None)
def vector(group: int, log_n: int, name: str) -> Vector:
    n = 1 << log_n
    w = M.domain_omega(log_n)
    ninv = pow(n, -1, R)
    assert name in names(group, log_n), name
    if name == "constant":
        s = [1] * n
        closed = {"fft": {0: n}, "ifft": {0: 1}}
    elif name == "all_infinity":
        s = [0] * n
        closed = {"fft": {}, "ifft": {}}
    elif name.startswith("delta_"):
        d = _delta_positions(n)[name]
        s = [1 if i == d else 0 for i in range(n)]
        closed = {"fft": {j: pow(w, j * d, R) for j in range(n)}, "ifft": {j: pow(w, -j * d, R) * ninv % R for j in range(n)}}
    elif name.startswith("frequency_"):
        k = _frequencies(n)[name]
        s = [pow(w, i * k, R) for i in range(n)]
        closed = {"fft": {(n - k) % n: n}, "ifft": {k: 1}}
    elif name == "two_frequencies":
        k = 5 % n   # the frequencies k and k + n/2 together: twice the single frequency on even i, cancelled on odd i
        s = [2 * pow(w, i * k, R) % R if i % 2 == 0 else 0 for i in range(n)]
        assert all((pow(w, i * k, R) + pow(w, i * (k + n // 2), R) - s[i]) % R == 0 for i in range(n))
        closed = {"fft": {(n - k) % n: n, (n - k - n // 2) % n: n}, "ifft": {k: 1, (k + n // 2) % n: 1}}
    else:
        h = n // 2
        prog = inputs.bases_progression_cpu(group, h, seed=0xED6E + 16 * log_n + group)
        zero = np.zeros_like(prog)
        if name == "mirrored_progression":
            neg = negate_records(group, prog)
            upper = prog.copy()
            upper[1::2] = neg[1::2]
            pts = np.concatenate([prog, upper])
        elif name == "half_infinite_low":
            pts = np.concatenate([zero, prog])
        else:
            assert name == "half_infinite_high"
            pts = np.concatenate([prog, zero])
        return Vector(name, group, log_n, None, pts, None)
    return Vector(name, group, log_n, s, _multiples_by_oracle(group, s), closed)


# ------------------------------------------------------------------------------------------------ the oracle's answers, computed once
@functools.lru_cache(maxsize=None)
def oracle(group: int, log_n: int, name: str, op: str) -> np.ndarray:
    """O.point_domain_op of the vector (EvaluationDomain<Point<G>>::{fft, ifft} + batch_normalization), shared by every test that needs it"""
    import oracle_lib as O

    out = O.point_domain_op(group, vector(group, log_n, name).points, log_n, op)
    out.setflags(write=False)
    return out
