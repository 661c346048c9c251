"""The choice rules of the leased pools without a GPU: a stand-alone C++ program (tests/cpp/test_pool_pick_host.cpp) over pool_pick.hpp.

For each of the four rules (the device buffers of the host-buffer entry points, the pinned buffers, the stages, the multiexp's small workspaces)
the program checks hand-written slot tables against the picks they must give -- empty pool, all busy, another device's idle slot, exact fit against
a larger fit, nothing fits, ties, and the small workspaces' cap just under, at and over it -- and 10 000 random tables of at most 12 slots against
a restatement of the loops the pools ran before the rules were pure functions.  It is built twice: plainly, and with AddressSanitizer and
UndefinedBehaviorSanitizer, which is sound here because the program is the whole process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_pool_pick_host.cpp")
CHECKS = 50 + 4 * 10000   # the hand-written tables and four rules over every random table


def _build(name, extra):
    """g++ tests/cpp/test_pool_pick_host.cpp -> build/<name>: host compiler only, nothing linked but the C++ runtime"""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    out = os.path.join(ROOT, "build", name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra"] + extra + [SRC, "-o", out])
    return out


@pytest.mark.parametrize("name,extra", [("test_pool_pick_host", []), ("test_pool_pick_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])],
                         ids=["plain", "asan-ubsan"])
def test_rules_match_the_tables_and_the_old_loops(name, extra):
    p = subprocess.run([_build(name, extra)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stderr == ""   # no sanitizer report, no failed check
    assert int(p.stdout.split()[1]) >= CHECKS
