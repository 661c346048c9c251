"""The G1 multiexp through the pair start of accumulate_run (csrc/msm_impl.hpp): a bucket whose run has at least two entries opens with
xyzzu_from_affine_pair instead of a copy and a full mixed addition.  tests/pair_start_check.py runs in ONE fresh child process with
MI355ZK_G1_PAIR=0, MI355ZK_MSM_SPLIT=0 and MI355ZK_MSM_C=10 (read once per process), so that small inputs take the lane-per-bucket
kernel over a bucket geometry the cases can aim at; every case there is compared exactly with the CPU oracle's multiexp, n <= 4096:

  bucket lengths 1, 2, 3, 4, 5, 8, 9 (the 4-entry index groups and their boundaries), in window 0 alone and in every window
  a bucket that opens with the same point twice (doubling), followed by 0, 1 and 3 further points; nine times the same point
  a bucket that opens with a pair that cancels -- by a negated base and by opposite signed digits -- followed by 0, 1 and 2 further
  points; the four-entry bucket P, -P, Q, -Q whose record is all zero
  the identity record as the first, the second and both leading entries of a bucket: skipped in dense mode, UnexpectedIdentity with the
  lowest such index in plain mode (what the loop reported before the pair start existed, and what the oracle reports)
  all exponents equal: one bucket takes the heavy path, entries j and j + 64 equal and opposite so that a lane's strided run opens with
  each exceptional pair
  a streamed host-buffer call in four chunks: CARRY launches over buckets that stay empty, are touched once, are touched in every chunk,
  carry an infinity record and meet their own point again
The child also shows, from the library's per-group launch records, that the streamed calls ran four lane-per-bucket launches and that the
all-equal calls left the lane-per-bucket launch for the heavy path: a planner change that turned them into plain-path cases fails here."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

CASES = (["sizes window 0", "sizes every window", "the same point nine times", "P, -P, Q, -Q: the all-zero record"]
         + ["doubling then %d" % k for k in (0, 1, 3)]
         + ["cancel by negated base then %d" % k for k in (0, 1, 2)] + ["cancel by opposite digits then %d" % k for k in (0, 1, 2)]
         + ["identity %s, %s" % (w, m) for w in ("first", "second", "first and second") for m in ("dense", "plain")]
         + ["heavy bucket, window 0", "heavy bucket, every window", "streamed, four chunks", "streamed, four chunks, random exponents", "bases used"])


@pytest.fixture(scope="module")
def child():
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, MI355ZK_G1_PAIR="0", MI355ZK_MSM_SPLIT="0", MI355ZK_MSM_C="10")
    p = subprocess.run([sys.executable, os.path.join(here, "pair_start_check.py")], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    return json.loads(p.stdout.strip().splitlines()[-1])


def test_the_child_ran_every_case(child):
    assert sorted(child) == sorted(CASES)


@pytest.mark.parametrize("case", CASES)
def test_case_matches_the_oracle(child, case):
    assert child[case]["ok"], (case, child[case])
