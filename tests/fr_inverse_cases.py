"""Cases and the big-int reference for the batch inversion of csrc/fr_inverse.hip (test_fr_inverse_host.py, test_gpu_fr_inverse.py).

Everything here works on the RAW words of Montgomery Fr elements: the raw word of a is A = a M mod r with M = 2^256 mod r, the raw word of
a^-1 is a^-1 M = M^2 A^-1 mod r, and a zero stays zero.  The reference inverts a vector with ONE modular inversion (prefix products in a plain
loop, pow(total, -1, r), back-substitution) and is cross-checked against pow(A, -1, r) on a sample, so the large sizes stay quick."""
import ctypes as C
import functools

import numpy as np

import bn254_model as M
import inputs

R = M.R_ORDER
MONT = (1 << 256) % R
MONT2 = MONT * MONT % R
PATTERNS = ("random", "all_one", "all_r_minus_1", "all_zero", "zero_first", "zero_last", "zero_at_run_boundary", "zero_at_tile_boundary",
            "one_run_zero", "one_tile_zero", "every_second_zero")
SIZE_NAMES = ("0", "1", "2", "run-1", "run", "run+1", "tile-1", "tile", "tile+1", "2tile+3")


def geometry(lib):
    run, tile, cw = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert lib.mi355zk_fr_inverse_geometry(C.byref(run), C.byref(tile), C.byref(cw)) == 0
    return run.value, tile.value, cw.value


def size(name: str, geom) -> int:
    run, tile, cw = geom
    return {"0": 0, "1": 1, "2": 2, "run-1": run - 1, "run": run, "run+1": run + 1, "tile-1": tile - 1, "tile": tile, "tile+1": tile + 1,
            "2tile+3": 2 * tile + 3, "largest": (cw + 1) * tile + 1}[name]


def rows(vals) -> np.ndarray:
    """raw words as ints -> (n, 4) u64"""
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in vals), dtype=np.uint64).reshape(-1, 4).copy()


def ints(a) -> list:
    b = np.ascontiguousarray(a).view(np.uint64).tobytes()
    return [int.from_bytes(b[i:i + 32], "little") for i in range(0, len(b), 32)]


def reference(raw) -> list:
    """raw words of the inverses, zero for zero"""
    idx = [i for i, a in enumerate(raw) if a]
    pre, acc = [], 1
    for i in idx:
        pre.append(acc)
        acc = acc * raw[i] % R
    j = pow(acc, -1, R) * MONT2 % R   # M^2 / (the product of the non-zero words)
    out = [0] * len(raw)
    for p, i in zip(reversed(pre), reversed(idx)):
        out[i] = p * j % R
        j = j * raw[i] % R
    for i in idx[::max(1, len(idx) // 64)] + idx[-1:]:
        assert out[i] == MONT2 * pow(raw[i], -1, R) % R
    return out


@functools.lru_cache(maxsize=None)
def elements(pattern: str, n: int, geom) -> tuple:
    """the raw words of the n inputs.  A position past the end moves to the last element, a range past the end covers everything."""
    run, tile, _ = geom
    if pattern == "all_one":
        return (MONT,) * n
    if pattern == "all_r_minus_1":
        return (R - 1,) * n
    if pattern == "all_zero":
        return (0,) * n
    a = [v if v else 1 for v in ints(inputs.random_fr_mont(n, seed=2000 + n % 991))] if n else []
    if pattern == "random" or n == 0:
        return tuple(a)
    at = {"zero_first": 0, "zero_last": n - 1, "zero_at_run_boundary": min(run, n - 1), "zero_at_tile_boundary": min(tile, n - 1)}
    if pattern in at:
        a[at[pattern]] = 0
    elif pattern in ("one_run_zero", "one_tile_zero"):
        w = run if pattern == "one_run_zero" else tile
        lo = w if n > w else 0
        for i in range(lo, min(lo + w, n)):
            a[i] = 0
    else:
        assert pattern == "every_second_zero"
        a[::2] = [0] * len(a[::2])
    return tuple(a)


@functools.lru_cache(maxsize=None)
def expected(pattern: str, n: int, geom):
    """((n, 4) u64 inverses, the number of zeros)"""
    a = elements(pattern, n, geom)
    return (rows(reference(a)) if n else np.zeros((0, 4), np.uint64)), sum(1 for v in a if not v)


def element_rows(pattern: str, n: int, geom) -> np.ndarray:
    return rows(elements(pattern, n, geom)) if n else np.zeros((0, 4), np.uint64)
