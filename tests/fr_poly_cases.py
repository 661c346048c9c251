"""Cases and the big-int reference for the polynomial division / evaluation of csrc/fr_poly.hip (test_fr_poly_host.py, test_gpu_fr_poly.py).

Everything here works on the RAW words of Montgomery Fr elements: with A = a * 2^256 mod r, the recurrence Q[i-1] = A[i] + z Q[i] mod r over
the raw words with the PLAIN point z yields the raw words of q, so the reference needs no conversion of the vectors."""
import ctypes as C
import functools
import random

import numpy as np

import bn254_model as M
import inputs

R = M.R_ORDER
MONT = (1 << 256) % R
Z_FIXED = 0x1D3C5B7A99887766554433221100FFEEDDCCBBAA0918273645546372819A0B1C % R
PATTERNS = ("random", "all_r_minus_1", "zero", "top_only", "bottom_only", "exact_multiple")
SIZE_NAMES = ("1", "2", "3", "run-1", "run", "run+1", "tile-1", "tile", "tile+1", "2tile+3")


def geometry(lib):
    run, tile, cw = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert lib.mi355zk_fr_poly_geometry(C.byref(run), C.byref(tile), C.byref(cw)) == 0
    return run.value, tile.value, cw.value


def size(name: str, geom) -> int:
    run, tile, cw = geom
    return {"1": 1, "2": 2, "3": 3, "run-1": run - 1, "run": run, "run+1": run + 1, "tile-1": tile - 1, "tile": tile, "tile+1": tile + 1,
            "2tile+3": 2 * tile + 3, "largest": (cw + 1) * tile + 1}[name]


def points(geom) -> list:
    """0, 1, 2, r - 1, a fixed random value, and elements of order RUN and TILE (z^RUN = 1 resp. z^TILE = 1: the scan multipliers become one)"""
    run, tile, _ = geom
    zs = [0, 1, 2, R - 1, Z_FIXED]
    for order in (run, tile):
        if (1 << M.FR_S) % order == 0:
            zs.append(pow(M.FR_ROOT_OF_UNITY, (1 << M.FR_S) // order, R))
    return zs


def kate_division(a, z):
    """kate_divison (sonic/util.rs:444-463) carried one step further: (q, remainder)"""
    q, cur = [0] * max(len(a) - 1, 0), 0
    for i in range(len(a) - 1, 0, -1):
        cur = (a[i] + z * cur) % R
        q[i - 1] = cur
    return q, ((a[0] + z * cur) % R if a else 0)


def horner(a, z):
    acc = 0
    for c in reversed(a):
        acc = (acc * z + c) % R
    return acc


def rows(vals) -> np.ndarray:
    """raw words as ints -> (n, 4) u64"""
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def ints(a) -> list:
    b = np.ascontiguousarray(a).view(np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def mont(v: int) -> np.ndarray:
    return rows([v % R * MONT % R])[0]


@functools.lru_cache(maxsize=None)
def coefficients(pattern: str, n: int, z: int = 0) -> tuple:
    """the raw words of n coefficients; only "exact_multiple" ((x - z) s(x): the remainder is exactly 0) depends on z"""
    if pattern == "random":
        return tuple(ints(inputs.random_fr_mont(n, seed=1000 + n % 997)))
    if pattern == "all_r_minus_1":
        return (R - 1,) * n
    if pattern == "zero":
        return (0,) * n
    if pattern == "top_only":
        return (0,) * (n - 1) + (Z_FIXED,)
    if pattern == "bottom_only":
        return (Z_FIXED,) + (0,) * (n - 1)
    assert pattern == "exact_multiple"
    if n == 1:
        return (0,)
    rnd = random.Random(n)
    s = [rnd.randrange(R) for _ in range(n - 1)]
    return tuple((p - z * c) % R for p, c in zip([0] + s, s + [0]))


@functools.lru_cache(maxsize=None)
def expected(pattern: str, n: int, z: int):
    """(q as (n - 1, 4) u64, remainder as (4,) u64) for coefficients(pattern, n, z) at z; the remainder is cross-checked against Horner"""
    a = coefficients(pattern, n, z if pattern == "exact_multiple" else 0)
    q, rem = kate_division(a, z)
    assert rem == horner(a, z) and (pattern != "exact_multiple" or rem == 0)
    return (rows(q) if q else np.zeros((0, 4), np.uint64)), rows([rem])[0]


def coefficient_rows(pattern: str, n: int, z: int) -> np.ndarray:
    return rows(coefficients(pattern, n, z if pattern == "exact_multiple" else 0))
