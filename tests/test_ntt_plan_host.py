"""The NTT's host arithmetic without a GPU: a stand-alone C++ program (tests/cpp/test_ntt_host.cpp) over ntt_plan.hpp.

Plan: for every request of the grid (log_n 1 .. 30 x batch 1, 3, 8 x the eight combinations of pre_g / post_c / post_g), under the default knobs and under
sixteen knob settings, the invariants of the plan: the passes' bits add up, launch geometry inside the kernels' limits (LDS, threads, 32-bit grid, the tile
permutation only where it is a bijection), every pass's loads and stores a permutation of [0, n) (enumerated with the kernel's own address arithmetic up to
2^16, by the strides above), every table a pass names among the plan's table requests and the one its scale mode reads, source and destination of every
pass; and one refused request per argument check.  That the planned values are the ones the driver computed before the split was shown by comparing the
`dump` mode byte for byte with the parent's (profiles/ntt_host_split.md)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GRID = 30 * 3 * 8       # requests
SETTINGS = 16           # the default knobs and fifteen settings


@pytest.fixture(scope="module")
def exe():
    """g++ tests/cpp/test_ntt_host.cpp -> build/test_ntt_host: host compiler only, nothing linked but the C++ runtime"""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    out = os.path.join(ROOT, "build", "test_ntt_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "cpp", "test_ntt_host.cpp"), "-o", out])
    return out


def test_plan_invariants_and_argument_errors(exe):
    p = subprocess.run([exe, "plan"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout[-4000:] + p.stderr[-2000:]
    assert int(p.stdout.split()[1]) >= GRID * SETTINGS + 3   # no request of the grid was skipped under any setting, and the refusals ran


def test_dump_names_every_request_and_no_pointer(exe):
    env = {k: v for k, v in os.environ.items() if not k.startswith("MI355ZK_NTT_")}
    p = subprocess.run([exe, "dump"], capture_output=True, text=True, env=env)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    assert len(lines) == GRID and all(" rc=0 " in l for l in lines)
    assert "0x" not in p.stdout
    # the flagship size: two passes of 1024-point rows on the wave-local kernel, the full table with the coset factors folded in
    l = [x for x in lines if x.startswith("log_n=20 batch=3 pre_g=1 post_c=0 post_g=0:")]
    assert len(l) == 1 and " R=2 b=10,10 " in l[0] and l[0].count("kernel=(ntt_pass_wl_kernel<10>)") == 2 and " fold=1 " in l[0]
    assert " preA=F.pre_stages " in l[0] and " twF=F.full" in l[0]
