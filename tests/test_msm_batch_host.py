"""The batched multiexp's host arithmetic without a GPU: a stand-alone C++ program (tests/cpp/test_msm_batch_host.cpp) over msm_plan.hpp and msm_join.hpp.

Plan: over n in {1, 33, 2^10, 20480, 2^16, 2^20} x B in {1, 2, 5, 16, 40, 300} x both groups -- B == 1 is today's plan field by field; the passes
msm_batch_split / msm_batch_pass cut cover 0 .. B exactly once and each is as large as the limits allow (one more vector is refused or past the workspace
budget); every pass plan has WL == B' * WD, a layout of non-overlapping regions that are multiples of 256, and holds every limit of the audit next to
MSM_BATCH_MAX_WINDOWS (msm_common.hpp); a batch with a table, chunks, a second base vector or window groups is refused.

Join: a pass of B vectors hands back B * WD * n_out window sums; the program fills them with s * G (random 64-bit s, one in five the zero record, as in
test_msm_join_host.py) and joins per vector (msm_join_batch), serially and on the helper threads.  Here every vector's affine point is compared with
    (sum_w 2^shift[w] * sum_k 2^e_k * s[v][w][k]  mod r) * G
over ITS slice of the records, with Python integers and the affine model (bn254_model)."""
import os
import subprocess

import pytest

import bn254_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.R_ORDER


@pytest.fixture(scope="module")
def exe():
    """g++ tests/cpp/test_msm_batch_host.cpp -> build/test_msm_batch_host: host compiler only, nothing linked but the C++ runtime"""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    out = os.path.join(ROOT, "build", "test_msm_batch_host")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", os.path.join(ROOT, "tests", "cpp", "test_msm_batch_host.cpp"), "-o", out, "-lpthread"])
    return out


def test_batch_plans_splits_and_refusals(exe):
    p = subprocess.run([exe, "plan"], capture_output=True, text=True)
    assert p.returncode == 0 and p.stdout.startswith("ok "), p.stdout[-4000:] + p.stderr[-2000:]
    assert int(p.stdout.split()[1]) >= 2 * 6 * 6 + 6   # the grid and the refused requests all ran


# (group, n, B): no running-sum level (2^10), two levels (2^16), a size that is no power of two; two vectors (the smallest pooled join) and more vectors than helpers
SHAPES = [(1, 1 << 10, 3), (1, 1 << 16, 2), (1, 20480, 9), (2, 1 << 10, 2), (2, 1 << 16, 3)]
CASES = [(s, serial) for s in SHAPES for serial in (0, 1)]


def _hex(v):
    return "%064x" % v


@pytest.fixture(scope="module")
def joined(exe, tmp_path_factory):
    """one run of the program over all cases: {(case id, vector): parsed output line}"""
    path = tmp_path_factory.mktemp("msm_batch_host") / "cases.txt"
    (x2, y2) = M.G2_GEN
    lines = ["g1 %s %s" % (_hex(M.G1_GEN[0]), _hex(M.G1_GEN[1])), "g2 %s %s %s %s" % (_hex(x2[0]), _hex(x2[1]), _hex(y2[0]), _hex(y2[1]))]
    for i, ((g, n, b), serial) in enumerate(CASES):
        lines.append("case %d %d %d %d %d %d" % (i, g, n, b, serial, 2000 + SHAPES.index((g, n, b))))   # serial and pooled joins see the same records
    path.write_text("\n".join(lines) + "\n")
    p = subprocess.run([exe, "join", str(path)], capture_output=True, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    out = {}
    for line in p.stdout.splitlines():
        f = line.split()
        assert f[0] == "case"
        kv = dict(t.split("=", 1) for t in f[2:] if "=" in t)
        kv["coords"] = f[f.index("result=") + 1:]
        out[(int(f[1]), int(kv["v"]))] = kv
    assert sorted(out) == [(i, v) for i, ((g, n, b), _) in enumerate(CASES) for v in range(b)]
    return out


def _expected_point(g, kv):
    ints = lambda key: [int(v) for v in kv[key].split(",")]
    wd, n_out = int(kv["WD"]), int(kv["n_out"])
    assert kv["rmul"] == "1"   # (ungrouped calls below 2^20 exponents take power-of-two windows)
    s, e_k, shift = ints("s"), ints("e_k"), ints("shift")
    assert len(s) == wd * n_out and len(e_k) == n_out and len(shift) == wd
    total = sum((1 << shift[w]) * sum(s[w * n_out + k] << e_k[k] for k in range(n_out)) for w in range(wd))
    return M.ec_mul(M.FQ_OPS if g == 1 else M.FQ2_OPS, M.G1_GEN if g == 1 else M.G2_GEN, total % R)


@pytest.mark.parametrize("idx", range(len(CASES)), ids=["g%d-n%d-B%d-%s" % (s + ("serial" if ser else "pooled",)) for s, ser in CASES])
def test_every_vector_joins_to_the_big_integer_sum_of_its_slice(joined, idx):
    (g, n, b), serial = CASES[idx]
    points = []
    for v in range(b):
        kv = joined[(idx, v)]
        assert kv["rc"] == "0" and int(kv["WL"]) == b * int(kv["WD"])
        want = _expected_point(g, kv)
        c = [int(x, 16) for x in kv["coords"]] if kv["coords"] != ["inf"] else None
        got = None if c is None else (c[0], c[1]) if g == 1 else ((c[0], c[1]), (c[2], c[3]))
        assert want is not None and got == want, (g, n, b, serial, v)
        points.append(got)
        # the helper threads took whole vectors exactly when asked to
        assert kv["parallel"] == ("0" if serial else "1"), (g, n, b, serial)
    assert len(set(points)) == b   # the slices differ: a join over the wrong slice would not pass
    # serial and pooled joins of the same records agree
    other = CASES.index(((g, n, b), 1 - serial))
    assert all(joined[(other, v)]["coords"] == joined[(idx, v)]["coords"] for v in range(b))
