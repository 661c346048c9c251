"""The limb and column bounds of the G1 bucket arithmetic, checked on the HOST by running the header's own lines: tests/cpp/test_u_bounds_host.cpp
instantiates the functions of csrc/fieldu.hpp and csrc/curveu.hpp that a G1 addition uses on limbs that carry worst-case intervals
(tests/cpp/u_interval.hpp) and reports every 64-bit column sum that can pass 2^64, every 32-bit limb expression that can wrap and every stated
precondition of u_mul / u_sqr / u_mul2 / u_sub that a caller does not meet, for operands ANYWHERE inside the stated invariants."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    out = os.path.join(ROOT, "build", "test_u_bounds_host")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "cpp", "test_u_bounds_host.cpp"), "-o", out])
    return out


def test_no_formula_can_overflow_within_its_preconditions(exe):
    p = subprocess.run([exe], capture_output=True, text=True)
    assert p.returncode == 0 and "\n0 violations" in p.stdout and "VIOLATION" not in p.stdout, p.stdout[-4000:] + p.stderr[-2000:]
    for what in ("xyzzu_add_mixed (negated)", "xyzzu_add_mixed (empty accumulator)", "xyzzu_double_affine", "xyzzu_from_affine_pair (the same point)", "xyzzr_add", "xyzzu_double"):
        assert what in p.stdout, what


def test_the_column_intervals_bite_u_sqr_of_uncarried_limbs(exe):
    p = subprocess.run([exe, "bite_sqr"], capture_output=True, text=True)
    assert p.returncode == 0 and "column sum can exceed 2^64" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]


def test_the_checker_bites_y3_with_x3_d_and_ny1_all_uncarried(exe):
    p = subprocess.run([exe, "bite"], capture_output=True, text=True)
    assert p.returncode == 0 and "REPORTED" in p.stdout and "u_mul2" in p.stdout, p.stdout[-2000:] + p.stderr[-2000:]
