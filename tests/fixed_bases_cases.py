"""Base sets, rows and oracle expectations for the fixed-bases linear-combination tests (CPU and GPU): out = first + sum_j k[j] * P_j over
bases with KNOWN logarithms, so that rows whose partial sums meet the exceptional cases of the group law can be written down.
TEST INFRASTRUCTURE."""
from __future__ import annotations

import numpy as np

import bn254_model as M
import fixed_base_cases as FB
import inputs
import oracle_lib as O

R = M.R_ORDER
FIRST_LOG = 0x1D3C5B7A99887766554433221100FFEEDDCCBBAA99887766554433221100F % R


def base_logs(n_bases: int, seed: int) -> list[int]:
    """u_j with P_j = u_j * G1: base 1 EQUALS base 0 and base 2 is the identity (u = 0), where the set is long enough"""
    u = FB.ints(inputs.random_scalars(max(n_bases, 1), seed=seed))[:n_bases]
    if n_bases >= 2:
        u[1] = u[0]
    if n_bases >= 3:
        u[2] = 0
    return u


def points(logs) -> np.ndarray:
    """log * G1 as (n, 8) u64 affine records (log 0: the all-zero record)"""
    if len(logs) == 0:
        return np.zeros((0, 8), np.uint64)
    return np.ascontiguousarray(O.G1.mul_many_affine(inputs.G1_GEN_RAW, FB.limbs(logs)))


def exceptional_rows(logs, first_log=FIRST_LOG) -> list[tuple[str, list[int]]]:
    """(name, row) over the bases of base_logs: the partial sum passes through the identity (two equal bases, k and r - k), equals the entry
    being added (two equal bases, 5 and 5: the doubling path), and the whole sum is -first (the all-zero record)"""
    n = len(logs)
    pad = lambda head: head + [0] * (n - len(head))  # noqa: E731
    rows = []
    if n >= 2:
        k = 0x2B3C4D5E6F708192A3B4C5D6E7F8091A2B3C4D5E6F708192A3B4C5D6E7F809 % R
        rows += [("cancel", pad([k, R - k])), ("double", pad([5, 5])), ("cancel_low", pad([1, R - 1]))]
    if n >= 1 and logs[0]:
        rows.append(("minus_first", pad([(R - first_log) * pow(logs[0], -1, R) % R])))
    if n >= 1:
        rows.append(("zeros", pad([])))
    return rows


def scalar_rows(rows) -> np.ndarray:
    """rows of ints -> (n, n_bases, 4) u64"""
    n_bases = len(rows[0]) if rows else 0
    return np.ascontiguousarray(np.array([[M.to_limbs(int(k)) for k in row] for row in rows], dtype=np.uint64).reshape(len(rows), n_bases, 4))


def want_lincomb(bases: np.ndarray, first, scalars: np.ndarray) -> np.ndarray:
    """the oracle's first + sum_j scalars[i][j] * bases[j] for every row, affine: O.G1.mul per column (mul_many_affine), add, to_affine"""
    n, n_bases = scalars.shape[0], bases.shape[0]
    cols = [O.G1.mul_many_affine(bases[j], np.ascontiguousarray(scalars[:, j])) if bases[j].any() else np.zeros((n, 8), np.uint64) for j in range(n_bases)]
    start = O.G1.from_affine(first) if first is not None else O.G1.from_affine(np.zeros(8, np.uint64))
    out = np.zeros((n, 8), np.uint64)
    for i in range(n):
        acc = start
        for col in cols:
            if col[i].any():
                acc = O.G1.add(acc, O.G1.from_affine(col[i]))
        out[i] = O.G1.to_affine(acc)
    return out
