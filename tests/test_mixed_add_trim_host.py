"""xyzzu_add_mixed, xyzzr_add and the bucket closing (csrc/curveu.hpp) on the HOST build, without a GPU: a stand-alone C++ program
(tests/cpp/test_mixed_add_trim_host.cpp) compiled with AddressSanitizer and UndefinedBehaviorSanitizer runs every case of
tests/mixed_add_trim_vectors.py -- accumulators injected at the edges of the invariants, operands 0, 1, p - 1, equal and opposite points,
chains of 80 additions -- and every coordinate is compared with the big-int formula.  Nothing is loaded into python.
The bounds the formulas rest on are tests/test_u_bounds_host.py; the device leg is tests/test_gpu_mixed_add_trim.py."""
import os
import subprocess

import pytest

import mixed_add_trim_vectors as TV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    out = os.path.join(ROOT, "build", "test_mixed_add_trim_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",      # the runtimes inside the program: nothing about it depends on what else the process loads
                           os.path.join(ROOT, "tests", "cpp", "test_mixed_add_trim_host.cpp"), "-o", out])
    return out


@pytest.fixture(scope="module")
def rows():
    return TV.cases()


def test_the_cases_cover_what_they_claim(rows):
    names = [n for n, _, _, _ in rows]
    for what in ("edge accumulator", "operand x=0 y=0", "operand x=1 y=p-1", "operand x=p-1 y=1", "empty accumulator", "equal x", "chain", "records at the edges", "the same point", "opposite points"):
        assert any(what in n for n in names), what
    assert sum(1 for n, inw, op, _ in rows if op == 0 and inw[1] >= 64) >= 3     # chains of at least 64 additions
    assert sum(1 for _, _, _, want in rows if want is None) >= 20     # P - P in every spelling
    top6, top2 = (6 * TV.Q - 1) >> 232, (2 * TV.Q - 1) >> 232
    assert TV.edge_values(6)[0] == 6 * TV.Q - 1 and TV.limbs(TV.edge_values(6)[3]) == [TV.MASK] * 8 + [top6 - 1] and TV.limbs(TV.edge_values(2)[4]) == [0] * 8 + [top2]


def test_host_build_against_the_model_under_sanitizers(exe, rows):
    text = "\n".join(" ".join("%x" % w for w in inw) for _, inw, _, _ in rows) + "\n"
    p = subprocess.run([exe], input=text, capture_output=True, text=True)     # the environment as inherited: a sanitizer report ends the program (rc != 0)
    assert p.returncode == 0 and not p.stderr, p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert len(lines) == len(rows)
    for (name, _, op, want), line in zip(rows, lines):
        TV.verify(name, op, [int(w, 16) for w in line.split()], want)
