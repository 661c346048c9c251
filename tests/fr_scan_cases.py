"""Cases and the big-int reference for the prefix scans of csrc/fr_scan.hip (test_fr_scan_host.py, test_gpu_fr_scan.py, test_gpu_ratio_scan.py,
test_gpu_grand_product.py).

Everything here works on the RAW words of Montgomery Fr elements: the raw word of a is A = a M mod r with M = 2^256 mod r, so the raw word of
a product is A B M^-1 mod r, the raw word of a sum A + B mod r, the raw word of one is M and zero stays zero.  The reference is the serial
chain in a plain loop."""
import ctypes as C
import functools

import numpy as np

import inputs
from fr_inverse_cases import MONT, MONT2, R, ints, rows  # noqa: F401  (the same helpers, re-exported for the tests)

MINV = pow(MONT, -1, R)
PATTERNS = ("random", "all_one", "all_r_minus_1", "zero_first", "zero_last", "zero_at_run_boundary", "zero_at_tile_boundary", "zero_in_last_tile")
SIZE_NAMES = ("0", "1", "2", "run-1", "run", "run+1", "tile-1", "tile", "tile+1", "2tile+3")
SUM, EXCLUSIVE = 1, 2   # MI355ZK_SCAN_SUM, MI355ZK_SCAN_EXCLUSIVE
MODES = (0, EXCLUSIVE, SUM, SUM | EXCLUSIVE)


def geometry(lib):
    run, tile, cw = C.c_uint32(), C.c_uint32(), C.c_uint32()
    assert lib.mi355zk_fr_scan_geometry(C.byref(run), C.byref(tile), C.byref(cw)) == 0
    return run.value, tile.value, cw.value


def size(name: str, geom) -> int:
    run, tile, cw = geom
    return {"0": 0, "1": 1, "2": 2, "run-1": run - 1, "run": run, "run+1": run + 1, "tile-1": tile - 1, "tile": tile, "tile+1": tile + 1,
            "2tile+3": 2 * tile + 3, "largest": (cw + 1) * tile + 1}[name]


def mont_mul(a: int, b: int) -> int:
    """the raw word of the product of the elements with raw words a and b"""
    return a * b * MINV % R


def reference(raw, num, flags: int):
    """(the raw words of the n outputs, the raw word of the aggregate of all n terms); the terms are raw[i], or num[i] raw[i] with num"""
    acc = 0 if flags & SUM else MONT
    out = []
    for i, a in enumerate(raw):
        if num is not None:
            a = num[i] * a * MINV % R
        if flags & EXCLUSIVE:
            out.append(acc)
        acc = (acc + a) % R if flags & SUM else acc * a * MINV % R
        if not flags & EXCLUSIVE:
            out.append(acc)
    return out, acc


@functools.lru_cache(maxsize=None)
def elements(pattern: str, n: int, geom, seed: int = 3000) -> tuple:
    """the raw words of the n inputs.  A position past the end moves to the last element."""
    run, tile, _ = geom
    if pattern == "all_one":
        return (MONT,) * n
    if pattern == "all_r_minus_1":
        return (R - 1,) * n
    a = [v if v else 1 for v in ints(inputs.random_fr_mont(n, seed=seed + n % 991))] if n else []
    if pattern == "random" or n == 0:
        return tuple(a)
    at = {"zero_first": 0, "zero_last": n - 1, "zero_at_run_boundary": min(run, n - 1), "zero_at_tile_boundary": min(tile, n - 1),
          "zero_in_last_tile": max(0, min((n - 1) // tile * tile + 1, n - 1))}
    a[at[pattern]] = 0
    return tuple(a)


def numerators(n: int, geom) -> tuple:
    """a second operand: random non-zero words from another seed"""
    return elements("random", n, geom, 4000)


@functools.lru_cache(maxsize=None)
def expected(pattern: str, n: int, geom, flags: int, with_num: bool = False):
    """((n, 4) u64 outputs, (4,) u64 total)"""
    out, total = reference(elements(pattern, n, geom), numerators(n, geom) if with_num else None, flags)
    return (rows(out) if n else np.zeros((0, 4), np.uint64)), rows([total])[0]


def element_rows(pattern: str, n: int, geom) -> np.ndarray:
    return rows(elements(pattern, n, geom)) if n else np.zeros((0, 4), np.uint64)


def numerator_rows(n: int, geom) -> np.ndarray:
    return rows(numerators(n, geom)) if n else np.zeros((0, 4), np.uint64)
