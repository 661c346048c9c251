"""The pinned-bases cache (bases_cache.hip) at its capacity: the least recently used vector of the device leaves, a vector larger than the
capacity runs uncached, and invalidate(nullptr) leaves nothing.  The capacity (MI355ZK_BASES_CACHE_GB) is read once per process, so
tests/bases_cache_check.py runs in a fresh child process, under its own time limit, with 0.0006 GB = 644 245 bytes: three pinned G1
vectors A, B, C of 4096 points (262 144 bytes each on the device: two fit, three do not) and D of 16384 points (1 MiB: above the
capacity), each multiplied by 4096 scalars and held against the CPU oracle."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

LIMIT = 120  # seconds; the child takes a few
COPY = 4096 * 64


def test_lru_eviction_at_capacity():
    here = os.path.dirname(os.path.abspath(__file__))
    env = {k: v for k, v in os.environ.items() if k not in ("MI355ZK_BASES_CACHE_IMPLICIT",)}
    env["MI355ZK_BASES_CACHE_GB"] = "0.0006"
    p = subprocess.run([sys.executable, os.path.join(here, "bases_cache_check.py")], capture_output=True, text=True, env=env, timeout=LIMIT)
    assert p.returncode == 0, (p.stdout[-2000:], p.stderr[-4000:])
    got = json.loads(p.stdout.strip().splitlines()[-1])
    held = lambda **kw: dict({"A": None, "B": None, "C": None, "D": None}, **kw)
    want = {
        "A": [True, held(A=COPY)],
        "B": [True, held(A=COPY, B=COPY)],
        "C": [True, held(B=COPY, C=COPY)],             # A, the least recently used, made room
        "B again": [True, held(B=COPY, C=COPY)],       # touched: now C is the older one
        "A again": [True, held(A=COPY, B=COPY)],       # C made room
        "D": [True, held(A=COPY, B=COPY)],             # larger than the capacity: uncached, nothing evicted for it
        "invalidate": [True, held()],
    }
    assert got == want
    assert list(got) == list(want)  # (the steps ran in this order)
