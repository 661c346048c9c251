#!/usr/bin/env python3
"""Fixed-base scalar multiplication on one MI355X, data resident in HBM: the window-table call (mi355zk_bn254_g{1,2}_fixed_base_mul_dev,
table already built) against mi355zk_bn254_g{1,2}_batch_mul_dev on the SAME scalars.  Both calls are timed to a synchronised stream
(batch_mul_dev synchronises itself), median of --iters runs after a warm-up of --warm calls and --warm-ms more, as tools/bench_ntt.py
does; the two results are compared record for record.  One JSON line per size."""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import phase2_bn254_amd as zk, inputs

ap = argparse.ArgumentParser()
ap.add_argument("--g1", default="16,20"); ap.add_argument("--g2", default="16,18"); ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--warm", type=int, default=3); ap.add_argument("--warm-ms", type=float, default=50.0)
a = ap.parse_args()
L = zk.lib.load(); w = zk.Worker(0)


def timed(fn):
    for _ in range(a.warm): fn()
    torch.cuda.synchronize()
    t_warm = time.perf_counter() + a.warm_ms * 1e-3
    while time.perf_counter() < t_warm: fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(a.iters):
        t = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
    return statistics.median(ts), min(ts)


for group, sizes in ((1, a.g1), (2, a.g2)):
    gen = np.ascontiguousarray(inputs.G1_GEN_RAW if group == 1 else inputs.G2_GEN_RAW)
    t0 = time.perf_counter(); tab = zk.FixedBaseTable(gen); torch.cuda.synchronize(); build_s = time.perf_counter() - t0
    old_fn = L.mi355zk_bn254_g1_batch_mul_dev if group == 1 else L.mi355zk_bn254_g2_batch_mul_dev
    for lg in [int(x) for x in sizes.split(",") if x]:
        n = 1 << lg
        k = torch.from_numpy(inputs.random_scalars(n, seed=77 + lg).view(np.int64)).cuda()
        old = torch.empty((n, 8 * group), dtype=torch.int64, device="cuda")
        new = [None]

        def run_old():
            assert old_fn(C.c_void_p(old.data_ptr()), gen.ctypes.data_as(C.c_void_p), C.c_void_p(k.data_ptr()), n, None) == 0

        def run_new():
            new[0] = tab.mul(k)

        t_old, min_old = timed(run_old)
        t_new, min_new = timed(run_new)
        print(json.dumps({"group": group, "log_n": lg, "table_build_ms": round(build_s * 1e3, 2), "batch_mul_ms": round(t_old * 1e3, 3), "batch_mul_min_ms": round(min_old * 1e3, 3),
                          "fixed_base_ms": round(t_new * 1e3, 3), "fixed_base_min_ms": round(min_new * 1e3, 3), "speedup": round(t_old / t_new, 2),
                          "fixed_base_Mpoint_per_s": round(n / t_new / 1e6, 1), "batch_mul_Mpoint_per_s": round(n / t_old / 1e6, 1),
                          "equal": bool(torch.equal(old, new[0]))}), flush=True)
