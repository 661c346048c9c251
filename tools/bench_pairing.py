#!/usr/bin/env python3
"""Pairing products on one MI355X, data resident in HBM: mi355zk_bn254_pairing_product_dev over 2^k single-pair groups (--singles) and over
one group of 2^k pairs (--group), timed to a synchronised stream -- median and minimum of --iters calls after --warm calls and --warm-ms
more of the same shape -- then, in a run of its own with the library's event timers on (mi355zk_prof_*), the three stages separately.
Beside them the single-thread host product (mi355zk_bn254_pairing_product) on this box's CPU, per pairing.  Inputs are random multiples of
the generators (distinct per pair); the first and last device results are compared with the host product.  One JSON line per shape."""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import phase2_bn254_amd as zk, inputs

ap = argparse.ArgumentParser()
ap.add_argument("--singles", default="6,10,14,16"); ap.add_argument("--group", default="14"); ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warm", type=int, default=2); ap.add_argument("--warm-ms", type=float, default=200.0); ap.add_argument("--host-pairings", type=int, default=50)
a = ap.parse_args()
L = zk.lib.load(); w = zk.Worker(0)
STAGES = ("pairing_miller", "pairing_product", "pairing_final_exp")


def points(n, seed):
    out = []
    for group, fn in ((1, L.mi355zk_bn254_g1_batch_mul_dev), (2, L.mi355zk_bn254_g2_batch_mul_dev)):
        gen = np.ascontiguousarray(inputs.G1_GEN_RAW if group == 1 else inputs.G2_GEN_RAW)
        k = torch.from_numpy(inputs.random_scalars(n, seed=seed + group).view(np.int64)).cuda()
        p = torch.empty((n, 8 * group), dtype=torch.int64, device="cuda")
        assert fn(C.c_void_p(p.data_ptr()), gen.ctypes.data_as(C.c_void_p), C.c_void_p(k.data_ptr()), n, None) == 0
        out.append(p)
    torch.cuda.synchronize()
    return out


def timed(fn):
    for _ in range(a.warm): fn()
    torch.cuda.synchronize()
    t_warm = time.perf_counter() + a.warm_ms * 1e-3
    while time.perf_counter() < t_warm: fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(a.iters):
        t = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
    return statistics.median(ts), min(ts)


def stages(fn):
    """per-stage milliseconds of ONE call, events on (a run of its own: the event records cost host time)"""
    L.mi355zk_prof_reset(); L.mi355zk_prof_enable(1)
    fn(); torch.cuda.synchronize()
    L.mi355zk_prof_enable(0)
    out = {}
    for name in STAGES:
        ms, cnt = C.c_double(), C.c_long()
        L.mi355zk_prof_get(name.encode(), C.byref(ms), C.byref(cnt))
        out[name + "_ms"] = round(ms.value, 3)
    return out


def host_product(g1, g2):
    h1, h2 = np.ascontiguousarray(g1.cpu().numpy().view(np.uint64)), np.ascontiguousarray(g2.cpu().numpy().view(np.uint64))
    out = np.zeros(48, dtype=np.uint64)
    assert L.mi355zk_bn254_pairing_product(out.ctypes.data_as(C.c_void_p), h1.ctypes.data_as(C.c_void_p), h2.ctypes.data_as(C.c_void_p), h1.shape[0]) == 0
    return out


g1, g2 = points(a.host_pairings, 5)
t = time.perf_counter()
for i in range(a.host_pairings): host_product(g1[i:i + 1], g2[i:i + 1])
host_ms = (time.perf_counter() - t) / a.host_pairings * 1e3
print(json.dumps({"host_single_thread_ms_per_pairing": round(host_ms, 3), "device": torch.cuda.get_device_name(0)}), flush=True)

shapes = [("singles", int(x)) for x in a.singles.split(",") if x] + [("one_group", int(x)) for x in a.group.split(",") if x]
for kind, lg in shapes:
    n = 1 << lg
    g1, g2 = points(n, 100 + lg)
    ptr = None if kind == "singles" else torch.tensor([0, n], dtype=torch.int32, device="cuda")
    res = [None]

    def run():
        res[0] = zk.pairing.pairing_product(g1, g2, ptr)

    med, best = timed(run)
    got = res[0].cpu().numpy().view(np.uint64)
    if kind == "singles":
        ok = bool(np.array_equal(got[0], host_product(g1[:1], g2[:1])) and np.array_equal(got[-1], host_product(g1[-1:], g2[-1:])))
    else:
        ok = bool(np.array_equal(got[0], host_product(g1, g2))) if n <= (1 << 14) else None
    row = {"shape": kind, "log_pairs": lg, "ms": round(med * 1e3, 3), "min_ms": round(best * 1e3, 3), "pairings_per_s": round(n / med, 1),
           "matches_host": ok}
    row.update(stages(run))
    print(json.dumps(row), flush=True)
