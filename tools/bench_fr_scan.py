#!/usr/bin/env python3
"""The prefix scans (csrc/fr_scan.hip) on one MI355X, per size n and number of rows:
  product, sum      mi355zk_bn254_fr_scan_dev, out of place, inclusive
  ratio             mi355zk_bn254_fr_ratio_scan_dev with numerators, exclusive product, into its own array
  three_calls       what the ratio call fuses: batch_inverse_dev, mul_assign_dev, fr_scan_dev
  mul_assign        mi355zk_bn254_fr_mul_assign_dev over the same rows * n elements: the yardstick (96 B per element, one product)
  host_product      ONE host thread running mi355zk_selftest_fr_scan over one row (the reference runs this chain serially); one sample
Both run lengths: the shipped library (16 elements per lane) and tools/bin/libmi355zk_scan_run8.so (`make scan_run8`).  A library is chosen when it is loaded, so
each is measured by a CHILD process of this script (--child; MI355ZK_SO names the library), one after the other on the same device, each with
its own mul_assign and its own warm-up.  The VGPR counts come from the compile (`make scan_resources` writes the compiler's resource remarks
to tools/bin/fr_scan_run{8,16}.resources.txt; read when present).
Device rows: median, min, max over --rounds samples of --inner back-to-back calls between two synchronisations, after --warm-ms of work.
Writes a markdown file to --md and one JSON line to stdout."""
import argparse, ctypes as C, json, os, re, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, nargs="+", default=[12, 16, 20, 24]); ap.add_argument("--rows", type=int, nargs="+", default=[1, 16])
ap.add_argument("--max-log-total", type=int, default=24); ap.add_argument("--host-max-log-n", type=int, default=22)
ap.add_argument("--rounds", type=int, default=7); ap.add_argument("--inner", type=int, default=5); ap.add_argument("--warm-ms", type=float, default=50.0)
ap.add_argument("--md", default=None); ap.add_argument("--child", action="store_true")
A = ap.parse_args()
RUN8_SO = os.path.join(ROOT, "tools", "bin", "libmi355zk_scan_run8.so")
ROWS = ("product", "sum", "ratio", "three_calls", "mul_assign")


def stats(samples):
    s = sorted(samples)
    return {"median_ms": round(statistics.median(s) * 1e3, 4), "min_ms": round(s[0] * 1e3, 4), "max_ms": round(s[-1] * 1e3, 4), "samples": len(s)}


def chk(rc):
    assert rc == 0, rc


def timed(rows, warm):
    """rows: name -> callable; alternated inside every round, so they see the same clocks"""
    import torch

    for fn in rows.values(): fn()
    t_warm = time.perf_counter() + A.warm_ms * 1e-3
    while time.perf_counter() < t_warm: warm()
    torch.cuda.synchronize()
    samples = {k: [] for k in rows}
    for _ in range(A.rounds):
        for name, fn in rows.items():
            fn(); torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(A.inner): fn()
            torch.cuda.synchronize(); samples[name].append((time.perf_counter() - t) / A.inner)
    return {k: stats(s) for k, s in samples.items()}


def child():
    import numpy as np, torch
    import phase2_bn254_amd as zk, inputs

    L, vp = zk.lib.load(), C.c_void_p
    geom = [C.c_uint32() for _ in range(3)]
    chk(L.mi355zk_fr_scan_geometry(*[C.byref(g) for g in geom]))
    out = {"library": os.path.basename(zk.lib.SO_PATH), "geometry": [g.value for g in geom], "cases": []}
    for log_n in A.log_n:
        n = 1 << log_n
        for rows in A.rows:
            if log_n + (rows - 1).bit_length() > A.max_log_total: continue
            host = inputs.random_fr_mont(n * rows, seed=90 + log_n)
            den = torch.from_numpy(host.view(np.int64)).cuda()
            num = den.flip(0).contiguous()
            o1, o2, o3, terms, x = (torch.empty_like(den) for _ in range(5))
            x.copy_(den)
            p = lambda t: vp(t.data_ptr())   # noqa: E731
            EX = zk.lib.SCAN_EXCLUSIVE

            def three_calls():
                chk(L.mi355zk_bn254_fr_batch_inverse_dev(p(terms), p(den), n * rows, None, None))
                chk(L.mi355zk_bn254_fr_mul_assign_dev(p(terms), p(num), n * rows, None))
                chk(L.mi355zk_bn254_fr_scan_dev(p(o3), n, p(terms), n, n, rows, EX, None, None))

            calls = {"product": lambda: chk(L.mi355zk_bn254_fr_scan_dev(p(o1), n, p(den), n, n, rows, 0, None, None)),
                     "sum": lambda: chk(L.mi355zk_bn254_fr_scan_dev(p(o1), n, p(den), n, n, rows, zk.lib.SCAN_SUM, None, None)),
                     "ratio": lambda: chk(L.mi355zk_bn254_fr_ratio_scan_dev(p(o2), n, p(num), n, p(den), n, n, rows, EX, None, None, None)),
                     "three_calls": three_calls,
                     "mul_assign": lambda: chk(L.mi355zk_bn254_fr_mul_assign_dev(p(x), p(num), n * rows, None))}
            res = timed(calls, lambda: (calls["mul_assign"](), calls["product"]()))
            calls["ratio"](); three_calls(); torch.cuda.synchronize()
            assert torch.equal(o2, o3)   # the timed calls are the right ones
            for k in ("product", "sum", "ratio", "three_calls"):
                res[k + "_over_mul_assign"] = round(res[k]["median_ms"] / res["mul_assign"]["median_ms"], 2)
            if rows == 1 and log_n <= A.host_max_log_n:
                h_out = np.empty_like(host)
                t = time.perf_counter()
                chk(L.mi355zk_selftest_fr_scan(h_out.ctypes.data_as(vp), host.ctypes.data_as(vp), None, n, 0, None))
                res["host_product"] = stats([time.perf_counter() - t])
                calls["product"](); torch.cuda.synchronize()
                assert np.array_equal(o1.cpu().numpy().view(np.uint64), h_out)
            out["cases"].append({"log_n": log_n, "rows": rows, "rows_ms": res})
            del den, num, o1, o2, o3, terms, x
            torch.cuda.empty_cache()
    print("CHILD_JSON " + json.dumps(out))


def run_child(so):
    env = dict(os.environ)
    if so: env["MI355ZK_SO"] = so
    argv = [sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(A.rounds), "--inner", str(A.inner), "--warm-ms", str(A.warm_ms),
            "--max-log-total", str(A.max_log_total), "--host-max-log-n", str(A.host_max_log_n), "--rows"] + [str(v) for v in A.rows] + ["--log-n"]
    p = subprocess.run(argv + [str(v) for v in A.log_n], env=env, capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("CHILD_JSON ")][-1][len("CHILD_JSON "):])


def resources(path):
    """kernel -> (VGPRs, AGPRs, waves per SIMD) from the compiler's -Rpass-analysis=kernel-resource-usage remarks"""
    if not os.path.exists(path): return None
    rows = {}
    pat = r"Function Name: (\S+).*?VGPRs: (\d+).*?AGPRs: (\d+).*?Occupancy \[waves/SIMD\]: (\d+)"
    for m in re.finditer(pat, open(path).read(), re.S):
        k = re.search(r"fr_scan_(\w+?)_kernel", m.group(1))
        if not k or k.group(1) in ("identity", "carry"): continue
        name = "%s %s%s" % (k.group(1), "sum" if "ScanSum" in m.group(1) else "product", " +num" if re.search(r"Scan(?:Sum|Product)ELb1", m.group(1)) else "")
        rows.setdefault(name, (int(m.group(2)), int(m.group(3)), int(m.group(4))))
    return rows


if A.child:
    child()
    sys.exit(0)
variants = {"run_16": run_child(None)}
if os.path.exists(RUN8_SO): variants["run_8"] = run_child(RUN8_SO)
import torch   # noqa: E402  (after the children: this process opens the device only now)
res_tab = {k: resources(os.path.join(ROOT, "tools", "bin", "fr_scan_%s.resources.txt" % k.replace("_", ""))) for k in ("run_16", "run_8")}
out = {"device": torch.cuda.get_device_name(0), "rounds": A.rounds, "inner": A.inner, "warm_ms": A.warm_ms, "scan": variants, "resources": res_tab}
print(json.dumps(out))
if A.md:
    cell = lambda r: "%.4g (%.4g .. %.4g)" % (r["median_ms"], r["min_ms"], r["max_ms"])   # noqa: E731
    with open(A.md, "w") as f:
        f.write("| n | rows | run | " + " | ".join(c + " ms" for c in ROWS) + " | product / mul_assign | sum / mul_assign | ratio / mul_assign | three_calls / ratio | host_product ms |\n")
        f.write("|---" * (len(ROWS) + 8) + "|\n")
        for name, v in variants.items():
            for c in v["cases"]:
                r = c["rows_ms"]
                f.write("| 2^%d | %d | %d | " % (c["log_n"], c["rows"], v["geometry"][0]) + " | ".join(cell(r[k]) for k in ROWS) +
                        " | %.3g | %.3g | %.3g | %.3g | %s |\n" % (r["product_over_mul_assign"], r["sum_over_mul_assign"], r["ratio_over_mul_assign"],
                                                                   r["three_calls"]["median_ms"] / r["ratio"]["median_ms"],
                                                                   "%.4g" % r["host_product"]["median_ms"] if "host_product" in r else "-"))
        f.write("\n| kernel | " + " | ".join("%s VGPRs / AGPRs / waves per SIMD" % k for k in res_tab) + " |\n|---|---|---|\n")
        names = sorted({n for t in res_tab.values() if t for n in t})
        for n in names:
            f.write("| %s | " % n + " | ".join("%d / %d / %d" % t[n] if t and n in t else "not measured yet" for t in res_tab.values()) + " |\n")
