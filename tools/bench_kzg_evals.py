#!/usr/bin/env python3
"""The batch inversion (csrc/fr_inverse.hip) and the evaluation-form KZG steps (csrc/fr_evals.hip, kzg.py) on one MI355X.

Table 1, batch_inverse against the pointwise kernel, per size n: variant (a) -- three launches, one inversion per call: the shipped library --
and variant (b) -- one launch, one inversion per tile: tools/bin/libmi355zk_inv_one_launch.so (`make inv_one_launch`).  A library is chosen
when it is loaded, so each variant is measured by a CHILD process of this script (--child; MI355ZK_SO names the library), one after the other
on the same device, each with its own mul_assign as the yardstick and its own warm-up.
Table 2, the routes at 2^--route-log-n, in this process with the shipped library:
  divide_evals     mi355zk_bn254_fr_evals_divide_dev, B points              against  ifft + kzg.divide + one fft per quotient
  open_evals_many  kzg.open_evals_many, B points                            against  ifft + kzg.open_many
Device rows: median, min, max over --rounds samples of --inner back-to-back calls between two synchronisations, after --warm-ms of work (an
idle MI355X needs tens of ms to raise its clocks: profiles/r05_ntt_warmup_ab.txt).  The open rows are one sample each after a warm-up call.
Writes a markdown file to --md and one JSON line to stdout."""
import argparse, ctypes as C, json, os, statistics, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, nargs="+", default=[12, 16, 20, 24]); ap.add_argument("--route-log-n", type=int, default=20)
ap.add_argument("--points", type=int, nargs="+", default=[1, 16]); ap.add_argument("--rounds", type=int, default=9)
ap.add_argument("--inner", type=int, default=10); ap.add_argument("--warm-ms", type=float, default=50.0)
ap.add_argument("--no-open", action="store_true"); ap.add_argument("--md", default=None); ap.add_argument("--child", action="store_true")
A = ap.parse_args()
ONE_LAUNCH_SO = os.path.join(ROOT, "tools", "bin", "libmi355zk_inv_one_launch.so")


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
    """batch_inverse and mul_assign at every size with the library this process loaded"""
    import numpy as np, torch
    import phase2_bn254_amd as zk, inputs

    L, vp = zk.lib.load(), C.c_void_p
    geom = [C.c_uint32() for _ in range(3)]
    chk(L.mi355zk_fr_inverse_geometry(*[C.byref(g) for g in geom]))
    out = {"library": os.path.basename(zk.lib.SO_PATH), "geometry": [g.value for g in geom], "sizes": {}}
    for log_n in A.log_n:
        n = 1 << log_n
        host = inputs.random_fr_mont(n, seed=70 + log_n)
        a = torch.from_numpy(host.view(np.int64)).cuda()
        inv, x, y = torch.empty_like(a), a.clone(), a.clone()
        rows = {"batch_inverse": lambda: chk(L.mi355zk_bn254_fr_batch_inverse_dev(vp(inv.data_ptr()), vp(a.data_ptr()), n, None, None)),
                "mul_assign": lambda: chk(L.mi355zk_bn254_fr_mul_assign_dev(vp(x.data_ptr()), vp(y.data_ptr()), n, None))}
        res = timed(rows, lambda: (rows["mul_assign"](), rows["batch_inverse"]()))
        chk(L.mi355zk_bn254_fr_mul_assign_dev(vp(inv.data_ptr()), vp(a.data_ptr()), n, None))   # a * (1 / a) == 1: the timed kernel is the right one
        one = np.frombuffer(((1 << 256) % zk.ceremony._R_ORDER).to_bytes(32, "little"), dtype=np.uint64)
        assert (inv.cpu().numpy().view(np.uint64) == one).all()
        res["inverse_over_mul_assign"] = round(res["batch_inverse"]["median_ms"] / res["mul_assign"]["median_ms"], 2)
        out["sizes"][str(log_n)] = res
        del a, inv, x, y
        torch.cuda.empty_cache()
    print("CHILD_JSON " + json.dumps(out))


def run_child(so):
    env = dict(os.environ)
    if so: env["MI355ZK_SO"] = so
    argv = [sys.executable, os.path.abspath(__file__), "--child", "--rounds", str(A.rounds), "--inner", str(A.inner), "--warm-ms", str(A.warm_ms), "--log-n"]
    p = subprocess.run(argv + [str(v) for v in A.log_n], env=env, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-4000:]
    return json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("CHILD_JSON ")][-1][len("CHILD_JSON "):])


def routes():
    import numpy as np, torch
    import phase2_bn254_amd as zk, inputs

    K, L, vp, R = zk.kzg, zk.lib.load(), C.c_void_p, zk.ceremony._R_ORDER
    worker = zk.Worker(0)
    TAU = 0x2F0E1D2C3B4A59687796A5B4C3D2E1F00F1E2D3C4B5A69788796A5B4C3D2E1F % R
    mont = lambda v: np.frombuffer((v % R * (1 << 256) % R).to_bytes(32, "little"), dtype=np.uint64).copy()   # noqa: E731
    log_n = A.route_log_n
    n = 1 << log_n
    evals = torch.from_numpy(inputs.random_fr_mont(n, seed=60 + log_n).view(np.int64)).cuda()
    lsrs = None
    if not A.no_open:
        pw = torch.empty((n, 4), dtype=torch.int64, device="cuda")
        chk(L.mi355zk_bn254_fr_powers_dev(vp(pw.data_ptr()), mont(TAU).ctypes.data_as(vp), mont(1).ctypes.data_as(vp), n, None))
        g1 = zk.FixedBaseTable(zk.ceremony.G1_ONE_RAW).mul(pw, montgomery=True)
        g2 = zk.FixedBaseTable(zk.ceremony.G2_ONE_RAW).mul(pw[:2].contiguous(), montgomery=True)
        lsrs = K.srs_lagrange(K.srs_from_points(g1, g2[0], g2[1]), log_n)

    def ifft(t):
        dom = zk.EvaluationDomain(t.clone(), log_n); dom.ifft(worker); return dom.into_coeffs()

    results = []
    for b in A.points:
        zs = [(TAU + 1 + 977 * j) % R for j in range(b)]
        z = np.concatenate([mont(v) for v in zs]); zp = z.ctypes.data_as(vp)
        q = torch.empty((b, n, 4), dtype=torch.int64, device="cuda"); qc = torch.zeros((b, n, 4), dtype=torch.int64, device="cuda")
        values = torch.empty((b, 4), dtype=torch.int64, device="cuda"); rem = torch.empty((b, 4), dtype=torch.int64, device="cuda")

        def coefficient_route():
            c = ifft(evals)
            chk(L.mi355zk_bn254_fr_poly_divide_dev(vp(qc.data_ptr()), n, vp(rem.data_ptr()), vp(c.data_ptr()), n, zp, b, None))   # (element n - 1 of a row is not rewritten: the timed calls transform what the last fft left there, the checked call starts from zeros)
            for j in range(b):
                dom = zk.EvaluationDomain(qc[j], log_n); dom.fft(worker)

        rows = {"divide_evals": lambda: chk(L.mi355zk_bn254_fr_evals_divide_dev(vp(q.data_ptr()), n, vp(values.data_ptr()), vp(evals.data_ptr()), log_n, zp, b, None)),
                "evaluate_evals": lambda: chk(L.mi355zk_bn254_fr_evals_divide_dev(None, n, vp(values.data_ptr()), vp(evals.data_ptr()), log_n, zp, b, None)),
                "ifft_divide_fft": coefficient_route}
        res = timed(rows, lambda: (rows["divide_evals"](), coefficient_route()))
        rows["divide_evals"](); qc.zero_(); coefficient_route(); torch.cuda.synchronize()
        assert torch.equal(q, qc) and torch.equal(values, rem)
        if lsrs is not None:
            K.open_evals_many(lsrs, evals, zs[:1]); K.open_many(lsrs, ifft(evals), zs[:1]); torch.cuda.synchronize()   # warm-up: the multiexp's workspaces
            t = time.perf_counter(); got = K.open_evals_many(lsrs, evals, zs); res["open_evals_many"] = stats([time.perf_counter() - t])
            t = time.perf_counter(); want = K.open_many(lsrs, ifft(evals), zs); res["ifft_open_many"] = stats([time.perf_counter() - t])
            assert got[0] == want[0] and np.array_equal(got[1], want[1])
        results.append({"log_n": log_n, "points": b, "rows": res})
        del q, qc
        torch.cuda.empty_cache()
    return results


if A.child:
    child()
    sys.exit(0)
variants = {"a_three_launches": run_child(None)}
if os.path.exists(ONE_LAUNCH_SO): variants["b_one_launch"] = run_child(ONE_LAUNCH_SO)
import torch   # noqa: E402  (after the children: this process opens the device only now)
route_rows = routes()
out = {"device": torch.cuda.get_device_name(0), "rounds": A.rounds, "inner": A.inner, "warm_ms": A.warm_ms, "batch_inverse": variants, "routes": route_rows}
print(json.dumps(out))
if A.md:
    cell = lambda r: "%.4g (%.4g .. %.4g)" % (r["median_ms"], r["min_ms"], r["max_ms"])   # noqa: E731
    with open(A.md, "w") as f:
        f.write("| n | variant | batch_inverse ms | mul_assign ms | batch_inverse / mul_assign per element |\n|---|---|---|---|---|\n")
        for log_n in A.log_n:
            for name, v in variants.items():
                r = v["sizes"][str(log_n)]
                f.write("| 2^%d | %s | %s | %s | %.3g |\n" % (log_n, name, cell(r["batch_inverse"]), cell(r["mul_assign"]), r["inverse_over_mul_assign"]))
        f.write("\n| n | B | " + " | ".join(c + " ms" for c in ("divide_evals", "evaluate_evals", "ifft_divide_fft", "open_evals_many", "ifft_open_many")) + " |\n|---|---|---|---|---|---|---|\n")
        for r in route_rows:
            f.write("| 2^%d | %d | " % (r["log_n"], r["points"]) +
                    " | ".join(cell(r["rows"][c]) if c in r["rows"] else "-" for c in ("divide_evals", "evaluate_evals", "ifft_divide_fft", "open_evals_many", "ifft_open_many")) + " |\n")
