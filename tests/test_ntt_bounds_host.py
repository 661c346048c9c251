"""The bound chain of the Fr transform's lazy butterflies, checked on the HOST by running the kernels' own lines: tests/cpp/test_ntt_bounds_host.cpp
instantiates csrc/ntt_butterfly.hpp -- the butterfly, the load- and store-side products, the closing reductions, the scale kernel's and the
table builders' lines -- on limbs that carry worst-case intervals (tests/cpp/u_interval.hpp) and derives, by induction over the stages from
the load state "canonical" alone, the value bound and limb size after every stage of every row length 2^1 .. 2^12, for every skip rule and
load / store mode the planner can emit.  Four modes substitute a broken schedule and must be REPORTED: the checker cannot pass vacuously.
Built a second time under AddressSanitizer + UndefinedBehaviorSanitizer (a stand-alone host program)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "test_ntt_bounds_host.cpp")
BASE = ["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas"]


@pytest.fixture(scope="module")
def exe():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    out = os.path.join(ROOT, "build", "test_ntt_bounds_host")
    subprocess.check_call(BASE + [SRC, "-o", out])
    return out


@pytest.fixture(scope="module")
def exe_san():
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    out = os.path.join(ROOT, "build", "test_ntt_bounds_host_san")
    subprocess.check_call(BASE + ["-fsanitize=undefined,address", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", SRC, "-o", out])
    return out


@pytest.fixture(scope="module")
def default_run(exe):
    return subprocess.run([exe], capture_output=True, text=True)


def test_no_stage_of_any_row_length_can_leave_its_bounds(default_run):
    p = default_run
    assert p.returncode == 0 and "\n0 violations" in p.stdout and "VIOLATION" not in p.stdout, p.stdout[-4000:] + p.stderr[-2000:]
    for log_np in range(1, 13):
        for pattern in ("plain, radix-2 rule", "plain, radix-4 / wave-local rule", "twisted (no skip)"):
            assert "rows of 2^%d, %s, pre " % (log_np, pattern) in p.stdout, (log_np, pattern)
    assert "combinations planned, all among them" in p.stdout
    for what in ("ntt_scale_kernel (a *= c * A * B)", "ntt_full_twiddle_kernel", "ntt_full_folded_kernel"):
        assert what in p.stdout, what


def _last_stage(out, head):
    block = out.split("  " + head + "   (skip_max")[1].split("\n  rows of")[0]
    return [float(v) for v in re.findall(r"stage \d+\*?\s+value <\s*([0-9.]+) p", block)][-1]


def test_the_derived_table_gives_the_documented_margins(default_run):
    """The figures ntt_butterfly.hpp and DESIGN.md quote: 30p after the ten stages of a 2^10 row that comes from a product at the load, 28p
    after the twelve of a 2^12 row (stage 2 not skipped), 2p + 2 s p on the twisted path; limbs never past 4 * 2^29 = 2^31."""
    out = default_run.stdout
    assert _last_stage(out, "rows of 2^10, plain, radix-4 / wave-local rule, pre 1") == 30.0
    assert _last_stage(out, "rows of 2^10, plain, radix-2 rule, pre 1") == 30.0
    assert _last_stage(out, "rows of 2^12, plain, radix-4 / wave-local rule, pre 2") == 28.0
    assert _last_stage(out, "rows of 2^10, twisted (no skip), pre 4") == 22.0
    assert _last_stage(out, "rows of 2^12, twisted (no skip), pre 4") == 26.0
    limbs = [float(v) for v in re.findall(r"limbs <\s*([0-9.]+) \* 2\^29", out)]
    assert limbs and max(limbs) == 4.0


@pytest.mark.parametrize("mode,report", [
    ("bite_skip3", ("> precondition: value(b)", "u_to_std_lt32p precondition: value")),
    ("bite_carry8", ("u_mul_shoup precondition: limb", "limb expression can wrap")),
    ("bite_sub2", (", 1> precondition: value(b)",)),
    ("bite_unhooked", ("u_to_std_lt2p precondition: value < inf p",)),
])
def test_the_checker_reports_a_broken_schedule(exe, mode, report):
    p = subprocess.run([exe, mode], capture_output=True, text=True)
    assert p.returncode == 0 and "REPORTED" in p.stdout and any(r in p.stdout for r in report), p.stdout[-3000:] + p.stderr[-2000:]


def test_the_checker_runs_clean_under_sanitizers(exe_san, default_run):
    p = subprocess.run([exe_san], capture_output=True, text=True)      # the environment as inherited: a sanitizer report ends the program (rc != 0)
    assert p.returncode == 0 and p.stdout == default_run.stdout, p.stdout[-2000:] + p.stderr[-4000:]
    for mode in ("bite_skip3", "bite_carry8", "bite_sub2", "bite_unhooked"):
        q = subprocess.run([exe_san, mode], capture_output=True, text=True)
        assert q.returncode == 0, q.stdout[-2000:] + q.stderr[-4000:]
