"""The host-buffer entry points' host arithmetic without a GPU: a stand-alone C++ program (tests/cpp/test_host_plan.cpp) over host_plan.hpp.

plan: the density plan (rank / select / the first exponent without a base against a bit-by-bit count, for n_scalars 0 .. 1000 x density_bits shorter,
equal, longer x all-ones / all-zero / random / FullDensity x the bases running out before, inside, after the map x two offsets), the chunk schedule
(seven sizes x bases travelling or not x five knob settings), the cells of the multi-device call (four sizes x 1, 2, 3, 8 devices x six
MI355ZK_MULTI_PLAN settings x FullDensity and a random map with an Eof), the join rule (every assignment of six outcomes to three cells x three
sets of error indices x with and without a planned Eof, against a restatement of the rule), range_parts, weight_cuts and shared_shift at their
thresholds, the argument rules and the knobs' parsing.  That the planned values are the ones the drivers computed before the split was shown
by comparing the `dump` mode byte for byte with the parent's (profiles/host_entry_split.md)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DENSITY = 7 * 3 * 4 * 3 * 2
CUTS = 7 * 2            # per knob setting
CUT_SETTINGS = 5
CELLS = 4 * 4 * 2       # per MI355ZK_MULTI_PLAN setting
CELL_PLANS = 6
JOIN = 6 ** 3 * 3 * 2
WEIGHT = 7 * 4          # row_ptr arrays x device counts (dump); x five part counts in `plan`
KNOBS = [{}, {"MI355ZK_HOST_CHUNK_TEST": "64"}, {"MI355ZK_HOST_CHUNK_TEST": "512"}, {"MI355ZK_HOST_CHUNK_FIRST": "22"}, {"MI355ZK_HOST_CHUNK_GROWTH": "150"},
         {"MI355ZK_MULTI_PLAN": "2x1"}, {"MI355ZK_MULTI_PLAN": "1x2"}, {"MI355ZK_MULTI_PLAN": "2x2"}, {"MI355ZK_MULTI_PLAN": "9x9"}, {"MI355ZK_MULTI_PLAN": "0x1"}]


@pytest.fixture(scope="module")
def exe():
    """g++ tests/cpp/test_host_plan.cpp -> build/test_host_plan: host compiler only, nothing linked but the C++ runtime"""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    out = os.path.join(ROOT, "build", "test_host_plan")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "cpp", "test_host_plan.cpp"), "-o", out])
    return out


def clean_env(extra):
    env = {k: v for k, v in os.environ.items() if not k.startswith(("MI355ZK_HOST_", "MI355ZK_MULTI_", "MI355ZK_DENSE_", "MI355ZK_MSM_"))}
    env.update(extra)
    return env


def test_plan_invariants(exe):
    p = subprocess.run([exe, "plan"], capture_output=True, text=True, env=clean_env({}))
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout[-4000:] + p.stderr[-2000:]
    # no case of any grid was skipped
    assert int(p.stdout.split()[1]) >= DENSITY + CUTS * CUT_SETTINGS + CELLS * CELL_PLANS + JOIN + WEIGHT // 4 * 5


@pytest.mark.parametrize("knobs", KNOBS, ids=lambda k: "-".join("%s=%s" % (a.split("_", 1)[1], b) for a, b in k.items()) or "default")
def test_dump_names_every_case_and_no_pointer(exe, knobs):
    p = subprocess.run([exe, "dump"], capture_output=True, text=True, env=clean_env(knobs))
    assert p.returncode == 0, p.stderr[-2000:]
    lines = p.stdout.splitlines()
    count = lambda kind: sum(1 for l in lines if l.startswith(kind + " "))
    assert (count("cuts"), count("cells"), count("join"), count("weight")) == (CUTS, CELLS, JOIN, WEIGHT) and len(lines) == CUTS + CELLS + JOIN + WEIGHT
    assert "0x" not in p.stdout
    if not knobs:
        # the flagship call with its bases on the device: a 2^26 / 20 first chunk, each following one 1.8 x its predecessor, the last takes the rest
        l = [x for x in lines if x.startswith("cuts n=67108864 upload=0:")]
        assert len(l) == 1 and l[0].split(":")[1].split()[:3] == ["0", "3355456", "9395296"] and l[0].split()[-1] == "67108864"
        # eight devices, 2^20 + 17 exponents: eight ranges cut at multiples of 32, one cell each, on devices 0 .. 7
        l = [x for x in lines if x.startswith("cells n=1048593 devs=8 map=0 ")]
        assert len(l) == 1 and " pg=8 wg=1 " in l[0] and l[0].count("[") == 8 and "[7:917536-1048593/0@917541+131057]" in l[0]
