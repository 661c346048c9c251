#!/usr/bin/env python3
"""The Fr half of a KZG opening on one MI355X (csrc/fr_poly.hip) against the pointwise kernel, and open_many against the loop of open.

Rows per size n and point count B (median, min, max over --rounds samples; the device rows of one (n, B) alternate inside every round, so
they see the same clocks and the same neighbours):
  divide      mi355zk_bn254_fr_poly_divide_dev, B points            (launches 1, 2, 3)
  eval        mi355zk_bn254_fr_poly_eval_dev, B points              (launches 1, 2)
  mul_assign  mi355zk_bn254_fr_mul_assign_dev at the same n, the yardstick: 96 B per element, one product
  host_hook   mi355zk_selftest_fr_poly_divide on one thread (B = 1 only, one sample)
  open_many / open_loop   kzg.open_many with B points against B calls of kzg.open (one sample each after a warm-up; --no-open skips them)
Device rows time --inner back-to-back calls between two synchronisations.  Writes a markdown table to --md and one JSON line to stdout."""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import phase2_bn254_amd as zk, inputs

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20, 22]); ap.add_argument("--points", type=int, nargs="+", default=[1, 16])
ap.add_argument("--rounds", type=int, default=9); ap.add_argument("--inner", type=int, default=10); ap.add_argument("--warm-ms", type=float, default=50.0)
ap.add_argument("--no-open", action="store_true"); ap.add_argument("--md", default=None)
A = ap.parse_args()
L = zk.lib.load()
vp = C.c_void_p
R = zk.ceremony._R_ORDER
TAU = 0x2F0E1D2C3B4A59687796A5B4C3D2E1F00F1E2D3C4B5A69788796A5B4C3D2E1F % R


def mont(v):
    return np.frombuffer((v % R * (1 << 256) % R).to_bytes(32, "little"), dtype=np.uint64).copy()


def stats(samples):
    s = sorted(samples)
    return {"median_ms": round(statistics.median(s) * 1e3, 4), "min_ms": round(s[0] * 1e3, 4), "max_ms": round(s[-1] * 1e3, 4), "samples": len(s)}


def chk(rc):
    assert rc == 0, rc


def srs_for(n):
    """tau^i G, i < n, and H, tau H: the powers from fr_powers_dev, the points from the fixed-base tables"""
    pw = torch.empty((n, 4), dtype=torch.int64, device="cuda")
    chk(L.mi355zk_bn254_fr_powers_dev(vp(pw.data_ptr()), mont(TAU).ctypes.data_as(vp), mont(1).ctypes.data_as(vp), n, None))
    g1 = zk.FixedBaseTable(zk.ceremony.G1_ONE_RAW).mul(pw, montgomery=True)
    g2 = zk.FixedBaseTable(zk.ceremony.G2_ONE_RAW).mul(pw[:2].contiguous(), montgomery=True)
    return zk.kzg.srs_from_points(g1, g2[0], g2[1])


def run(log_n, b, srs):
    n = 1 << log_n
    host = inputs.random_fr_mont(n, seed=90 + log_n)
    a = torch.from_numpy(host.view(np.int64)).cuda()
    x, y = a.clone(), a.clone()
    q = torch.empty((b, n - 1, 4), dtype=torch.int64, device="cuda")
    rem = torch.empty((b, 4), dtype=torch.int64, device="cuda")
    zs = [(TAU + 1 + 977 * j) % R for j in range(b)]
    z = np.concatenate([mont(v) for v in zs]); zp = z.ctypes.data_as(vp)
    rows = {"divide": lambda: chk(L.mi355zk_bn254_fr_poly_divide_dev(vp(q.data_ptr()), n - 1, vp(rem.data_ptr()), vp(a.data_ptr()), n, zp, b, None)),
            "eval": lambda: chk(L.mi355zk_bn254_fr_poly_eval_dev(vp(rem.data_ptr()), vp(a.data_ptr()), n, zp, b, None)),
            "mul_assign": lambda: chk(L.mi355zk_bn254_fr_mul_assign_dev(vp(x.data_ptr()), vp(y.data_ptr()), n, None))}
    for fn in rows.values(): fn()
    t_warm = time.perf_counter() + A.warm_ms * 1e-3
    while time.perf_counter() < t_warm: rows["mul_assign"](); rows["divide"]()
    torch.cuda.synchronize()
    samples = {k: [] for k in rows}
    for _ in range(A.rounds):
        for name, fn in rows.items():
            fn(); torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(A.inner): fn()
            torch.cuda.synchronize(); samples[name].append((time.perf_counter() - t) / A.inner)
    res = {k: stats(s) for k, s in samples.items()}
    if b == 1:
        hq, hrem = np.empty((n - 1, 4), np.uint64), np.empty(4, np.uint64)
        t = time.perf_counter()
        chk(L.mi355zk_selftest_fr_poly_divide(hq.ctypes.data_as(vp), hrem.ctypes.data_as(vp), host.ctypes.data_as(vp), n, zp))
        res["host_hook"] = stats([time.perf_counter() - t])
        assert np.array_equal(hq, q[0].cpu().numpy().view(np.uint64)) and np.array_equal(hrem, rem[0].cpu().numpy().view(np.uint64))
    if srs is not None:
        zk.kzg.open_many(srs, a, zs[:1]); torch.cuda.synchronize()   # warm-up: the multiexp's workspaces at this size
        t = time.perf_counter(); many = zk.kzg.open_many(srs, a, zs); res["open_many"] = stats([time.perf_counter() - t])
        t = time.perf_counter(); loop = [zk.kzg.open(srs, a, v) for v in zs]; res["open_loop"] = stats([time.perf_counter() - t])
        assert many[0] == [v for v, _ in loop] and all(np.array_equal(many[1][j], w) for j, (_, w) in enumerate(loop))
    med = lambda k: res[k]["median_ms"]   # noqa: E731
    derived = {"divide_ns_per_coeff_point": round(med("divide") * 1e6 / (n * b), 4), "eval_ns_per_coeff_point": round(med("eval") * 1e6 / (n * b), 4),
               "mul_assign_ns_per_element": round(med("mul_assign") * 1e6 / n, 4),
               "divide_over_mul_assign_per_element": round(med("divide") / b / med("mul_assign"), 3),
               "apply_share_of_divide": round(1 - med("eval") / med("divide"), 3),
               "divide_GBs": round((64 * b + 32 * b) * n / (med("divide") * 1e-3) / 1e9, 1), "mul_assign_GBs": round(96 * n / (med("mul_assign") * 1e-3) / 1e9, 1)}
    return {"log_n": log_n, "points": b, "rows": res, "derived": derived}


geom = [C.c_uint32() for _ in range(3)]
chk(L.mi355zk_fr_poly_geometry(*[C.byref(g) for g in geom]))
results = []
for log_n in A.log_n:
    srs = None if A.no_open else srs_for(1 << log_n)
    for b in A.points:
        results.append(run(log_n, b, srs))
    del srs
    torch.cuda.empty_cache()
out = {"device": torch.cuda.get_device_name(0), "geometry": {"run": geom[0].value, "tile": geom[1].value, "carry_width": geom[2].value},
       "rounds": A.rounds, "inner": A.inner, "warm_ms": A.warm_ms, "results": results}
print(json.dumps(out))
if A.md:
    cols = ["divide", "eval", "mul_assign", "host_hook", "open_many", "open_loop"]
    with open(A.md, "w") as f:
        f.write("| n | B | " + " | ".join(c + " ms" for c in cols) + " | divide / mul_assign per element | apply share of divide | divide GB/s | mul_assign GB/s |\n")
        f.write("|---|---|" + "---|" * (len(cols) + 4) + "\n")
        for r in results:
            cell = lambda c: ("%.4g (%.4g .. %.4g)" % (r["rows"][c]["median_ms"], r["rows"][c]["min_ms"], r["rows"][c]["max_ms"])) if c in r["rows"] else "-"   # noqa: E731
            d = r["derived"]
            f.write("| 2^%d | %d | " % (r["log_n"], r["points"]) + " | ".join(cell(c) for c in cols) +
                    " | %.3g | %.3g | %.4g | %.4g |\n" % (d["divide_over_mul_assign_per_element"], d["apply_share_of_divide"], d["divide_GBs"], d["mul_assign_GBs"]))
