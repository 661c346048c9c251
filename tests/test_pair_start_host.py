"""xyzzu_from_affine_pair (csrc/curveu.hpp) on the HOST build, without a GPU: a stand-alone C++ program (tests/cpp/test_pair_start_host.cpp)
compiled with AddressSanitizer and UndefinedBehaviorSanitizer runs every case of tests/pair_start_vectors.py; the results are compared
with the big-int model (the affine sum exactly, the accumulator's limb bounds and domains, the record).  Nothing is loaded into python.
The device leg is tests/test_gpu_pair_start_op.py."""
import os
import subprocess

import pytest

import pair_start_vectors as PV

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    """g++ -fsanitize=undefined,address tests/cpp/test_pair_start_host.cpp -> build/test_pair_start_host: host compiler only"""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    out = os.path.join(ROOT, "build", "test_pair_start_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan",      # the runtimes inside the program: nothing about it depends on what else the process loads
                           os.path.join(ROOT, "tests", "cpp", "test_pair_start_host.cpp"), "-o", out])
    return out


def test_the_cases_cover_what_they_claim():
    rows = PV.cases()
    assert len(rows) >= 300 and all(len(w) == PV.IN_WORDS for _, w, _ in rows)
    names = [n for n, _, _ in rows]
    for what in ("random", "(doubles)", "(infinity)", "first", "second"):
        assert any(what in n for n in names), what
    edges = dict(PV.edge_points())
    # the generator (1, 2) has x = 1; y^2 = 3 and y^2 = 2 decide x = 0 and x = p - 1; every edge point is on the curve and not the identity
    assert "x=1" in edges and len(edges) == 6 and all(pt[1] != 0 for pt in edges.values())
    assert sum(1 for _, _, want in rows if want is None) >= 30
    text = open(os.path.join(ROOT, "include", "mi355zk.h")).read()
    assert "MI355ZK_DEVOP_G1_ADD_AFFINE_PAIR = MI355ZK_DEVOP_COUNT," in text      # PV.CODE


def test_host_build_against_the_model_under_sanitizers(exe):
    rows = PV.cases()
    text = "\n".join(" ".join("%x" % w for w in inw) for _, inw, _ in rows) + "\n"
    p = subprocess.run([exe], input=text, capture_output=True, text=True)     # the environment as inherited: a sanitizer report ends the program (rc != 0)
    assert p.returncode == 0 and not p.stderr, p.stderr[-4000:]
    lines = p.stdout.splitlines()
    assert len(lines) == len(rows)
    for (name, _, want), line in zip(rows, lines):
        PV.verify(name, [int(w, 16) for w in line.split()], want)
