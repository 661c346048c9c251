"""The multiexp's host arithmetic without a GPU: a stand-alone C++ program (tests/cpp/test_msm_host.cpp) over msm_plan.hpp and msm_join.hpp.

Join: for every case the program plans the call, fills the window sums the device would hand back with  h_wsums[wl][k] = s * G  (random 64-bit s, one in
five the zero record, as R-domain XYZZ records with ZZ != 1) and joins them; here the result is compared, as an affine point, with
    (sum_wl weight(w_lo + wl) * sum_k 2^e_k * s[wl][k]  mod r) * G,      weight(w) = 2^shift[w], B^w (mixed radix) or 1 (table mode),
computed with Python integers and the affine model (bn254_model).  Cases: G1 and G2, serial and parallel join, power-of-two and mixed-radix
windows, window groups, table mode, plans with and without the 2-D tail and without running-sum levels.  The exponents e_k[] and the shifts are the
ones the plan under test prints: what is checked independently is the JOIN given them.  e_k itself is checked for consistency with the level schedule (the
plan test below) and was compared byte for byte with the parent's derivation (profiles/msm_host_split.md), not against a second model.

Plan: the invariants of the workspace layout and the schedule over a grid of sizes (the SIZES of test_msm_digits_host.py, both groups, streamed calls of
1, 2 and 5 chunks, table mode), and one refused request per argument check."""
import os
import subprocess

import pytest

import bn254_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.R_ORDER


@pytest.fixture(scope="module")
def exe():
    """g++ tests/cpp/test_msm_host.cpp -> build/test_msm_host: host compiler only, nothing linked but the C++ runtime"""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    out = os.path.join(ROOT, "build", "test_msm_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "cpp", "test_msm_host.cpp"), "-o", out, "-lpthread"])
    return out


def test_plan_invariants_and_argument_errors(exe):
    p = subprocess.run([exe, "plan"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout[-4000:] + p.stderr[-2000:]
    assert int(p.stdout.split()[1]) >= 100   # the grid and the error cases all ran


# (n, wgroups, wgroup, table_c, final_max, no_tail2d): what each is there for
SHAPES = [
    (1 << 10, 1, 0, 0, 0, 0),     # power-of-two windows, no running-sum level (final_off == 1)
    (1 << 16, 1, 0, 0, 0, 0),     # power-of-two windows, two levels
    (20480, 1, 0, 0, 0, 0),       # power-of-two windows again (n < 2^20 ungrouped: the measured table), a size that is no power of two
    (1 << 26, 1, 0, 0, 0, 0),     # mixed radix (B = 5 * 2^19) at the flagship size (the join sees WL * n_out records whatever n is)
    (1 << 26, 2, 0, 0, 0, 0), (1 << 26, 2, 1, 0, 0, 0), (1 << 26, 4, 3, 0, 0, 0),   # window groups
    (40960, 2, 0, 0, 0, 0), (40960, 2, 1, 0, 0, 0), (40960, 4, 3, 0, 0, 0),   # (mixed radix too: B = 9 * 2^11 for two groups)
    (1 << 22, 2, 1, 0, 0, 0), (1 << 24, 4, 3, 0, 0, 0),   # a window group above the lowest one with power-of-two windows (its shift closes the join)
    (1 << 16, 1, 0, 17, 0, 0),    # table mode: ONE bucket set, weight 1
    (1 << 20, 1, 0, 20, 0, 0),    # table mode with the 2-D tail (G1: row_bits > 0)
    (1 << 20, 1, 0, 20, 0, 1),    # ... and the same size without it
    (1 << 20, 1, 0, 0, 256, 0),   # a deeper level schedule
]
CASES = [(g, s, serial) for g in (1, 2) for s in SHAPES for serial in (0, 1)]


def _hex(v):
    return "%064x" % v


@pytest.fixture(scope="module")
def joined(exe, tmp_path_factory):
    """one run of the program over all cases: {case id: parsed output line}"""
    path = tmp_path_factory.mktemp("msm_host") / "cases.txt"
    (x2, y2) = M.G2_GEN
    lines = ["g1 %s %s" % (_hex(M.G1_GEN[0]), _hex(M.G1_GEN[1])), "g2 %s %s %s %s" % (_hex(x2[0]), _hex(x2[1]), _hex(y2[0]), _hex(y2[1]))]
    for i, (g, (n, wgroups, wgroup, table_c, final_max, no_tail), serial) in enumerate(CASES):
        seed = 1000 + SHAPES.index((n, wgroups, wgroup, table_c, final_max, no_tail)) * 2 + g     # serial and parallel join see the same records
        lines.append("case %d %d %d %d %d %d %d %d %d %d" % (i, g, n, wgroups, wgroup, table_c, serial, final_max, no_tail, seed))
    path.write_text("\n".join(lines) + "\n")
    p = subprocess.run([exe, "join", str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    out = {}
    for line in p.stdout.splitlines():
        f = line.split()
        assert f[0] == "case"
        kv = dict(t.split("=", 1) for t in f[2:] if "=" in t)
        kv["coords"] = f[f.index("result=") + 1:]
        out[int(f[1])] = kv
    assert sorted(out) == list(range(len(CASES)))
    return out


_expected = {}


def _expected_point(g, kv):
    ints = lambda key: [int(v) for v in kv[key].split(",")]
    WL, n_out, w_lo, rmul, rshift = (int(kv[k]) for k in ("WL", "n_out", "w_lo", "rmul", "rshift"))
    s, e_k, shift = ints("s"), ints("e_k"), ints("shift")
    assert len(s) == WL * n_out and len(e_k) == n_out
    total = 0
    for wl in range(WL):
        w = w_lo + wl
        weight = 1 if kv["tmode"] == "1" else (1 << shift[w]) if rmul == 1 else (rmul << rshift) ** w
        total += weight * sum(s[wl * n_out + k] << e_k[k] for k in range(n_out))
    key = (g, total % R)
    if key not in _expected:
        _expected[key] = M.ec_mul(M.FQ_OPS if g == 1 else M.FQ2_OPS, M.G1_GEN if g == 1 else M.G2_GEN, total % R)
    return _expected[key]


@pytest.mark.parametrize("idx", range(len(CASES)), ids=["g%d-n%d-wg%d.%d-t%d-f%d-nt%d-%s" % ((g,) + s + ("serial" if ser else "parallel",)) for g, s, ser in CASES])
def test_join_matches_the_big_integer_sum(joined, idx):
    g, shape, serial = CASES[idx]
    kv = joined[idx]
    assert kv["rc"] == "0"
    want = _expected_point(g, kv)
    c = [int(v, 16) for v in kv["coords"]] if kv["coords"] != ["inf"] else None
    got = None if c is None else (c[0], c[1]) if g == 1 else ((c[0], c[1]), (c[2], c[3]))
    assert want is not None and got == want, (g, shape, serial)


def test_cases_cover_the_schedules(joined):
    kvs = [joined[i] for i in range(len(CASES))]
    assert any(int(k["row_bits"]) > 0 for k in kvs) and any(int(k["row_bits"]) == 0 and k["tmode"] == "1" for k in kvs)   # with and without the 2-D tail
    assert any(k["n_levels"] == "0" and k["final_off"] == "1" for k in kvs)
    assert any(k["rmul"] != "1" and int(k["w_lo"]) > 0 for k in kvs) and any(k["rmul"] == "1" and int(k["WL"]) >= 4 and int(k["w_lo"]) > 0 for k in kvs)
    assert any(k["tmode"] == "1" for k in kvs)
    assert all(any(v == "0" for v in k["s"].split(",")) for k in kvs)   # every case holds zero records
    # the helper threads took the window sums exactly where they should: asked for (serial == 0) and at least four bucket sets
    for (g, shape, serial), k in zip(CASES, kvs):
        assert k["parallel"] == ("1" if not serial and int(k["WL"]) >= 4 else "0"), (g, shape, serial)
    ran = [k for k in kvs if k["parallel"] == "1"]
    assert any(k["rmul"] == "1" for k in ran) and any(k["rmul"] != "1" for k in ran)
