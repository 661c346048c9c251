"""Edge-value inputs through the device transform, byte for byte against closed forms (tests/ntt_edge_forms.py; no oracle up to 2^20): all zero,
all c = r - 1, all one, c at single indices, c on the even indices, and single tones -- whose transform is n c at one index and exactly 0 at every
other, so that every butterfly meets multiples of r, the closing reductions have to turn k r into 0 and subtractions meet equal operands.  The
random inputs of test_gpu_ntt.py never come near the 30p / 2^31 ceilings of the lazy butterfly chain (csrc/ntt_butterfly.hpp); these sit on them.
Sizes: every carry position and both parities of the stage count in one radix-2 pass (2^1 .. 2^10), two passes with the full table and the folded
scalings (2^11, 2^13, 2^18), the wave-local kernel and its twisted stage table (2^19, 2^20), long rows without a full table (2^21, 2^23), three
passes (2^24), the batched entry point, and the barrier radix-4 kernel in a child process."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bn254_model as M
import ntt_edge_forms as E
import oracle_lib as O

pytestmark = pytest.mark.gpu
OPS = E.OPS


def _run(zk, worker, a, op):
    dom = zk.EvaluationDomain.from_coeffs(a)
    getattr(dom, op)(worker)
    return dom.into_coeffs()


def _check(got, want, what):
    if not np.array_equal(got, want):
        bad = np.nonzero((got != want).any(axis=1))[0]
        raise AssertionError("%s: %d of %d elements differ, first at %d: got %s, want %s" % (what, len(bad), len(want), bad[0], [hex(int(w)) for w in got[bad[0]]],
                                                                                       [hex(int(w)) for w in want[bad[0]]]))


@pytest.mark.parametrize("log_n", [1, 2, 3, 4, 7, 8, 10, 11, 13, 18])
@pytest.mark.parametrize("op", OPS)
def test_every_edge_pattern_matches_its_closed_form(zk, worker, log_n, op):
    cs = E.cases(log_n, op)
    assert len(cs) >= 8      # 2^1: three constants, two deltas, two even / odd patterns, one tone
    for name, a, want in cs:
        _check(_run(zk, worker, a, op), want, (log_n, op, name))


@pytest.mark.parametrize("log_n", [19, 20])
@pytest.mark.parametrize("op", OPS)
def test_wave_local_sizes_match_their_closed_forms(zk, worker, log_n, op):
    """full tiles: the wave-local kernel, for coset_fft with the row twist in its stage table (no twiddle is one, no product skipped)"""
    cs = E.cases(log_n, op, which=["all c", "tone 1"])
    assert len(cs) == 2
    for name, a, want in cs:
        _check(_run(zk, worker, a, op), want, (log_n, op, name))


def _mont_powers(base, n):
    """[base^0 .. base^(n-1)] as Montgomery rows, by doubling through the oracle's field product"""
    mont = lambda v: np.array(M.to_limbs(v * M.MONT_R % M.R_ORDER), dtype=np.uint64)  # noqa: E731
    p = mont(1).reshape(1, 4)
    m = 1
    while m < n:
        p = np.concatenate([p, O.fe_mul_many(O.FR, p, np.tile(mont(pow(base, m, M.R_ORDER)), (m, 1))).reshape(-1, 4)])
        m *= 2
    return p[:n]


def _big_inputs(log_n):
    """all c, and the tone c omega^-i (stored integers: the Montgomery product of the rows omega^-i * 2^256 with the stored word c)"""
    n = 1 << log_n
    c_row = np.array(M.to_limbs(E.C), dtype=np.uint64)
    all_c = np.tile(c_row, (n, 1))
    tone = O.fe_mul_many(O.FR, _mont_powers(pow(M.domain_omega(log_n), -1, M.R_ORDER), n), all_c).reshape(-1, 4)
    return {"all c": all_c, "tone 1": tone}


@pytest.fixture(scope="module")
def big_inputs():
    memo = {}

    def get(log_n):
        if log_n not in memo:
            memo.clear()                     # one size at a time: 2^24 rows are 512 MiB
            memo[log_n] = _big_inputs(log_n)
        return memo[log_n]

    return get


@pytest.mark.parametrize("log_n,op", [(21, "fft"), (21, "coset_fft"), (21, "icoset_fft"), (23, "fft"), (23, "ifft"), (24, "fft")])
def test_sizes_beyond_the_closed_forms_match_the_oracle(zk, worker, big_inputs, log_n, op):
    """2^21: rows of 2^11, the column factor at the load and the row constants at the store (pre 4 / post 5); 2^23: rows of 2^12 (stage 2 not
    skipped); 2^24: three passes of 2^8.  Expected: the CPU oracle's transform of the same edge input, and the closed form where it is free."""
    n = 1 << log_n
    for name, a in big_inputs(log_n).items():
        got = _run(zk, worker, a, op)
        _check(got, O.fr_domain_op(a, log_n, op, log_cpus=3).reshape(-1, 4), (log_n, op, name))
        if op == "fft":                      # n c at index 0 (all c) or 1 (the tone), exactly 0 elsewhere
            peak = 0 if name == "all c" else 1
            assert [int(w) for w in got[peak]] == M.to_limbs(n * E.C % M.R_ORDER), (log_n, name)
            assert not got[:peak].any() and not got[peak + 1:].any(), (log_n, name)


@pytest.mark.parametrize("log_n", [12, 20])
@pytest.mark.parametrize("op", OPS)
def test_batched_entry_point_with_a_different_pattern_per_row(zk, worker, log_n, op):
    import torch

    cs = E.cases(log_n, op, which=["all c", "tone 1", "c at 1"])[:3]
    assert len(cs) == 3
    doms = [zk.EvaluationDomain(torch.from_numpy(a.view(np.int64)).cuda(), log_n) for _, a, _ in cs]
    getattr(zk.EvaluationDomain, op + "_many")(worker, doms)
    for (name, _, want), d in zip(cs, doms):
        _check(d.coeffs.cpu().numpy().view(np.uint64), want, (log_n, op, name, "batch of 3"))


@pytest.fixture(scope="module")
def barrier_child():
    """the barrier radix-4 kernel, which no default size reaches: MI355ZK_NTT_WAVELOCAL=0 is read once per process, hence a fresh child"""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MI355ZK_NTT_WAVELOCAL="0")
    p = subprocess.run([sys.executable, os.path.join(here, "ntt_edges_barrier_check.py")], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("op", OPS)
def test_barrier_radix4_kernel_on_a_tone(barrier_child, op):
    assert sorted(barrier_child) == sorted(OPS)
    assert barrier_child[op]["ok"], barrier_child[op]
