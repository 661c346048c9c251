"""The prefix scans of csrc/fr_scan.hpp without a GPU and without Python in the process: a stand-alone C++ program
(tests/cpp/test_fr_scan_host.cpp) runs the host side of the header -- the same lane routines as the kernels, in their grouping -- over the edge
sizes, products and sums, inclusive and exclusive, in place and out of place, with and without the second operand, with a zero in every
position of one run, and across two carry chunks, checking out[i] against out[i-1] step by step, the total and the elements past the end.  It
is built twice: plainly, and with AddressSanitizer and UndefinedBehaviorSanitizer, which is sound here because the program is the whole
process."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_fr_scan_host.cpp")
CHECKS = 1000


def _build(name, extra):
    """g++ tests/cpp/test_fr_scan_host.cpp -> build/<name>: host compiler only, nothing linked but the C++ runtime"""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    out = os.path.join(ROOT, "build", name)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Wno-unknown-pragmas"] + extra + [SRC, "-o", out])
    return out


@pytest.mark.parametrize("name,extra", [("test_fr_scan_host", []), ("test_fr_scan_host_san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])],
                         ids=["plain", "asan-ubsan"])
def test_chain_totals_and_bounds(name, extra):
    p = subprocess.run([_build(name, extra)], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout[-2000:] + p.stderr[-4000:]
    assert p.stderr == ""   # no sanitizer report, no failed check
    assert int(p.stdout.split()[1]) >= CHECKS
