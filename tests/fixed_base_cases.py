"""Scalars for the fixed-base window-table tests (CPU and GPU): the edges of the signed 8-bit recoding of csrc/fixed_base.hpp.
TEST INFRASTRUCTURE."""
from __future__ import annotations

import numpy as np

import bn254_model as M
import inputs

R = M.R_ORDER


def limbs(vals) -> np.ndarray:
    """ints < 2^256 -> (n, 4) little-endian u64"""
    return np.array([M.to_limbs(int(v)) for v in vals], dtype=np.uint64).reshape(-1, 4)


def ints(arr) -> list[int]:
    return [M.from_limbs([int(x) for x in row]) for row in np.asarray(arr, dtype=np.uint64).reshape(-1, 4)]


def edge_scalars() -> list[int]:
    """canonical scalars at the edges of the recoding: carries through every window, digits +-127 / 128, the largest top digit, and the one
    scalar whose partial sum EQUALS the entry added last (k = 2 e - r with e = 48 * 2^248: the low windows sum to e - r)"""
    all_7f, all_80 = int("7f" * 32, 16), int("80" * 32, 16)
    out = [0, 1, R - 1, R - 2, (R - 1) // 2, all_7f % (1 << 253), all_80 % (1 << 253), all_7f % R, all_80 % R, int("2f" + "ff" * 31, 16)]
    assert all(k < R for k in out)
    nbytes = 32
    while int("ff" * nbytes, 16) >= R:       # every byte 0xff, up to the largest such value below r
        nbytes -= 1
    out += [int("ff" * b, 16) for b in range(1, nbytes + 1)]
    for w in range(32):
        for j in (1, 127, 128, 129, 255):
            if (j << (8 * w)) < R:
                out.append(j << (8 * w))
    out.append(2 * (48 << 248) - R)
    assert 0 < out[-1] < R
    return out


def test_scalars(n_random: int, seed: int) -> np.ndarray:
    """the edge list followed by n_random uniform scalars, (n, 4) u64"""
    return np.concatenate([limbs(edge_scalars()), inputs.random_scalars(n_random, seed=seed)])


test_scalars.__test__ = False   # (a helper, not a test)
