"""Linear combinations over a set of fixed G1 bases on the HOST (no GPU): the new symbols, the slice plan (host arithmetic), one row of
the combination through the program of the kernels (mi355zk_selftest_fixed_bases_lincomb) against the oracle's mul / add / to_affine --
the rows whose partial sums meet the exceptional cases of the group law above all -- and the argument checks of every entry point."""
import ctypes as C
import os

import numpy as np
import pytest

import fixed_base_cases as FB
import fixed_bases_cases as FBS
import inputs
import oracle_lib as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = FBS.R
NEW_SYMBOLS = ("mi355zk_fixed_bases_table_bytes", "mi355zk_fixed_bases_plan", "mi355zk_bn254_g1_fixed_bases_build_dev",
               "mi355zk_bn254_g1_fixed_bases_lincomb_dev", "mi355zk_selftest_fixed_bases_lincomb")


@pytest.fixture(scope="module")
def lib(zk):
    return zk.lib.load()


def _p(a):
    return None if a is None else np.ascontiguousarray(a).ctypes.data_as(C.c_void_p)


def _lincomb(lib, bases, first, row):
    """rc, record: one row (ints) over (n_bases, 8) bases"""
    out = np.zeros(8, np.uint64)
    ks = FB.limbs(row) if len(row) else np.zeros((0, 4), np.uint64)
    rc = lib.mi355zk_selftest_fixed_bases_lincomb(_p(bases) if len(row) else None, len(row), _p(first), _p(ks) if len(row) else None, _p(out))
    return rc, out


def test_symbols_are_declared_exported_and_bound(zk, lib):
    header = open(os.path.join(ROOT, "include", "mi355zk.h")).read()
    for name in NEW_SYMBOLS:
        assert name + "(" in header, name
        assert name in zk.lib.SIGNATURES, name
        fn = getattr(lib, name)
        assert fn.argtypes is not None and len(fn.argtypes) == len(zk.lib.SIGNATURES[name][1]), name
    assert "MI355ZK_FIXED_BASES_LANE_TARGET %du" % zk.lib.FIXED_BASES_LANE_TARGET in header


def test_plan(zk, lib):
    target = zk.lib.FIXED_BASES_LANE_TARGET
    for n in (1, 2, 255, 1 << 10, 1 << 20):
        for n_bases in (0, 1, 2, 31, 1000):
            sl, ns = C.c_size_t(0), C.c_size_t(0)
            assert lib.mi355zk_fixed_bases_plan(n, n_bases, C.byref(sl), C.byref(ns)) == 0
            sl, ns = sl.value, ns.value
            assert sl >= 1, (n, n_bases)
            assert (ns - 1) * sl < n_bases <= ns * sl, (n, n_bases, sl, ns)
            assert n * ns < 1 << 31, (n, n_bases)
            if n >= target and n_bases:
                assert ns == 1, (n, n_bases)
            if n_bases:
                assert n * (ns - 1) < target, (n, n_bases, sl, ns)     # never more slices than the target asks for
    # one row over a thousand bases is cut: that is what the slices are for
    sl, ns = C.c_size_t(0), C.c_size_t(0)
    assert lib.mi355zk_fixed_bases_plan(1, 1000, C.byref(sl), C.byref(ns)) == 0 and ns.value > 1
    assert lib.mi355zk_fixed_bases_plan((1 << 31) - 1, 1000, C.byref(sl), C.byref(ns)) == 0 and ns.value == 1


@pytest.mark.parametrize("n_bases", [0, 1, 2, 5])
def test_host_lincomb_matches_the_oracle(lib, n_bases):
    logs = FBS.base_logs(n_bases, seed=9300 + n_bases)
    bases = FBS.points(logs)
    point = FBS.points([FBS.FIRST_LOG])[0]
    edge = FB.edge_scalars()
    rows = [row for _, row in FBS.exceptional_rows(logs)]
    if n_bases:
        # the edge list dealt out over the columns, so that every column meets every edge; n_bases = 1: the whole list, one scalar a row
        step = 1 if n_bases == 1 else 7
        rows += [[edge[(i + 3 * j) % len(edge)] for j in range(n_bases)] for i in range(0, len(edge), step)]
    else:
        rows = [[]]
    scalars = FBS.scalar_rows(rows) if n_bases else np.zeros((1, 0, 4), np.uint64)
    for first in (None, np.zeros(8, np.uint64), point):
        want = FBS.want_lincomb(bases, first, scalars)
        for i, row in enumerate(rows):
            rc, got = _lincomb(lib, bases, first, row)
            assert rc == 0
            assert np.array_equal(got, want[i]), (n_bases, first is None, [hex(k) for k in row])


def test_exceptional_rows_give_what_the_group_law_says(lib):
    """the expectations stated directly, not through the oracle: (k, r - k) over two equal bases is `first`; (5, 5) is 10 P; a sum of -first
    is the all-zero record; an identity base contributes nothing whatever its scalar"""
    logs = FBS.base_logs(5, seed=9305)
    bases = FBS.points(logs)
    assert np.array_equal(bases[0], bases[1]) and not bases[2].any()
    first = FBS.points([FBS.FIRST_LOG])[0]
    named = dict(FBS.exceptional_rows(logs))
    for name in ("cancel", "cancel_low"):
        assert np.array_equal(_lincomb(lib, bases, first, named[name])[1], first), name
        assert not _lincomb(lib, bases, None, named[name])[1].any(), name
    ten_p = O.G1.mul_many_affine(bases[0], FB.limbs([10]))[0]
    assert np.array_equal(_lincomb(lib, bases, None, named["double"])[1], ten_p)
    assert not _lincomb(lib, bases, first, named["minus_first"])[1].any()
    assert np.array_equal(_lincomb(lib, bases, first, [0, 0, R - 1, 0, 0])[1], first)        # the identity base
    k = FB.ints(inputs.random_scalars(1, seed=9306))[0]
    assert np.array_equal(_lincomb(lib, bases, None, [0, 0, k, 7, 0])[1], O.G1.mul_many_affine(bases[3], FB.limbs([7]))[0])


def test_bad_arguments_are_refused_without_a_device(lib):
    sl, ns = C.c_size_t(0), C.c_size_t(0)
    assert lib.mi355zk_fixed_bases_table_bytes(0) == 0
    assert lib.mi355zk_fixed_bases_table_bytes(3) == 3 * 4096 * 64
    assert lib.mi355zk_fixed_bases_table_bytes(1 << 62) == 0 and lib.mi355zk_fixed_bases_table_bytes(1 << 19) == 0   # overflow / too many entries
    assert lib.mi355zk_fixed_bases_plan(4, 4, None, C.byref(ns)) == 3
    assert lib.mi355zk_fixed_bases_plan(4, 4, C.byref(sl), None) == 3
    assert lib.mi355zk_fixed_bases_plan(1 << 31, 4, C.byref(sl), C.byref(ns)) == 3
    gen = np.ascontiguousarray(inputs.G1_GEN_RAW)
    off = gen.copy()
    off[4:] = O.fe_add(0, off[4:], off[4:])                                                   # (x, 2 y): on no curve
    fake = C.c_void_p(0x1000)                                                                 # never dereferenced: every call below returns first
    build = lib.mi355zk_bn254_g1_fixed_bases_build_dev
    assert build(None, 0, None, 0, None) == 0                                                 # nothing to build
    assert build(None, 4096 * 64, _p(gen), 1, None) == 3
    assert build(fake, 4096 * 64, None, 1, None) == 3
    assert build(fake, 4096 * 64 - 1, _p(gen), 1, None) == 3                                  # a short table
    assert build(fake, 2 * 4096 * 64, _p(np.stack([gen, off])), 2, None) == 3                 # a base off the curve
    comb = lib.mi355zk_bn254_g1_fixed_bases_lincomb_dev
    assert comb(None, None, 0, None, None, 0, 0, None) == 0                                   # n == 0
    assert comb(None, fake, 1, None, fake, 1, 0, None) == 3
    assert comb(fake, None, 1, None, fake, 1, 0, None) == 3
    assert comb(fake, fake, 1, None, None, 1, 0, None) == 3
    assert comb(fake, fake, 1, None, fake, 1 << 31, 0, None) == 3
    assert comb(fake, fake, 4, None, fake, 1 << 30, 1, None) == 3                             # n times the slice count
    hook = lib.mi355zk_selftest_fixed_bases_lincomb
    k, out = np.zeros(4, np.uint64), np.zeros(8, np.uint64)
    assert hook(_p(gen), 1, None, _p(k), None) == 3
    assert hook(None, 1, None, _p(k), _p(out)) == 3
    assert hook(_p(gen), 1, None, None, _p(out)) == 3
    assert hook(_p(off), 1, None, _p(k), _p(out)) == 3                                        # off the curve
    assert hook(None, 0, None, None, _p(out)) == 0 and not out.any()                          # no base, no first: the identity
