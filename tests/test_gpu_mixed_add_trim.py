"""The G1 multiexp over the trimmed bucket addition (csrc/curveu.hpp: the sign of the added point applied inside R, the un-carried D): small
calls in which every changed line runs.  tests/mixed_add_trim_check.py runs in ONE fresh child process with MI355ZK_G1_PAIR=0,
MI355ZK_MSM_SPLIT=0 and MI355ZK_MSM_C=6 (read once per process): 32 buckets per window, so 2^12 and 2^14 points give every bucket more than
a hundred entries of mixed sign.  Every case is compared by affine point with the CPU oracle's multiexp; the bucket array
of one 2^12 call (mi355zk_selftest_g1_msm_buckets_dev: the records the accumulate stage left, before the reduction) is compared word for word with the
same buckets (the index lists that call reports) accumulated by the big-int model of the formulas as they were before the trims."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CASES = ["2^12 points", "2^14 points", "repeated and negated bases", "P + P, -Q - Q, P - P and a one-entry run", "one-entry runs", "identity records, dense", "bucket array, word for word",
         "skewed exponents, the heavy path", "streamed, three chunks"]


@pytest.fixture(scope="module")
def child():
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MI355ZK_G1_PAIR="0", MI355ZK_MSM_SPLIT="0", MI355ZK_MSM_C="6")
    p = subprocess.run([sys.executable, os.path.join(here, "mixed_add_trim_check.py")], env=env, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_the_child_ran_every_case(child):
    assert sorted(child) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_case_matches_the_oracle(child, case):
    assert child[case]["ok"], (case, child[case])
