#!/usr/bin/env python3
"""Strided affine records against packed records on the host-buffer multiexp (include/mi355zk.h: mi355zk_bn254_g{1,2}_msm_strided):
the same points as pairing's 72 / 136-byte `G1Affine` / `G2Affine` records and as packed 64 / 128-byte records, the variants ALTERNATED
inside one process after a warm-up.  Prints one JSON line; never bench.py's `value`.
  python tools/bench_strided.py [--cases g1:20 g1:26 g2:20] [--reps 5] [--pack-stats DIR]
  python tools/bench_strided.py --pack-only            one unpinned strided call per case (what a `rocprofv3 --kernel-trace --stats` run
                                                       wraps, so that records_pack moved exactly n * (stride + packed record) bytes)
--pack-stats DIR: the directory of that rocprofv3 run; the records_pack rows of its *kernel_stats.csv go into the line."""
import argparse
import csv
import ctypes as C
import glob
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import inputs  # noqa: E402
import phase2_bn254_amd as zk  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--cases", nargs="+", default=["g1:20", "g1:26", "g2:20"])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--pack-only", action="store_true")
ap.add_argument("--pack-stats", default=None)
a = ap.parse_args()
L = zk.lib.load()
w = zk.Worker(0)
dev = torch.device("cuda", 0)


def host_inputs(group, log_n, seed):
    n = 1 << log_n
    k = bench.gen_scalars(n, seed, dev)
    s = bench.gen_scalars(n, seed + 1, dev)
    b = torch.empty((n, 8 * group), dtype=torch.int64, device=dev)
    gen = np.ascontiguousarray(inputs.G1_GEN_RAW if group == 1 else inputs.G2_GEN_RAW)
    fn = L.mi355zk_bn254_g1_batch_mul_dev if group == 1 else L.mi355zk_bn254_g2_batch_mul_dev
    assert fn(C.c_void_p(b.data_ptr()), gen.ctypes.data_as(C.c_void_p), C.c_void_p(k.data_ptr()), n, None) == 0
    torch.cuda.synchronize()
    hb, hs = b.cpu().numpy().view(np.uint64), s.cpu().numpy().view(np.uint64)
    del b, s, k
    torch.cuda.empty_cache()
    limbs = 4 * group
    sb = (zk.StridedBases.g1_affine_rust if group == 1 else zk.StridedBases.g2_affine_rust)(hb[:, :limbs], hb[:, limbs:], None, pad=0xA5)
    return hb, hs, sb


def timed(bases, hs):
    t = time.perf_counter()
    r = zk.multiexp(w, (bases, 0), zk.FullDensity(), hs).wait()
    return (time.perf_counter() - t) * 1e3, bytes(r.tobytes())


def summary(ts):
    return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}


out = {"entry": "mi355zk_bn254_g{1,2}_msm_strided vs mi355zk_bn254_g{1,2}_msm (host buffers, pageable)", "reps": a.reps, "cases": {}}
for case in a.cases:
    g, ln = case.split(":")
    group, log_n = int(g[1]), int(ln)
    hb, hs, sb = host_inputs(group, log_n, seed=90 + log_n + group)
    if a.pack_only:
        timed(sb, hs)
        out["cases"][case] = {"strided_unpinned_calls": 1, "records": 1 << log_n, "stride": sb.stride}
        del hb, hs, sb
        continue
    G = __import__("oracle_lib").G1 if group == 1 else __import__("oracle_lib").G2
    aff = lambda r: bytes(np.asarray(G.to_affine(np.frombuffer(r, dtype=np.uint64))).tobytes())  # noqa: E731
    timed(hb[:4096], hs[:4096])          # warm-up: streams, workspaces, staging buffers of both variants (not the cache)
    timed(zk.StridedBases(sb.data[:4096], group, sb.x_off, sb.y_off, sb.inf_off), hs[:4096])
    res = set()
    unp_p, unp_s = [], []
    for _ in range(a.reps):              # unpinned: every call uploads its bases
        t, r = timed(hb, hs); unp_p.append(t); res.add(aff(r))
        t, r = timed(sb, hs); unp_s.append(t); res.add(aff(r))
    zk.pin_bases(hb)
    zk.pin_bases(sb)
    first_p, r = timed(hb, hs); res.add(aff(r))
    first_s, r = timed(sb, hs); res.add(aff(r))
    pin_p, pin_s = [], []
    for _ in range(a.reps):              # pinned, steady: only the exponents travel
        t, r = timed(hb, hs); pin_p.append(t); res.add(aff(r))
        t, r = timed(sb, hs); pin_s.append(t); res.add(aff(r))
    zk.unpin_bases(hb)
    zk.unpin_bases(sb)
    pp, ps = statistics.median(pin_p), statistics.median(pin_s)
    up, us = statistics.median(unp_p), statistics.median(unp_s)
    spread = max(max(pin_p) - min(pin_p), max(pin_s) - min(pin_s)) / pp
    out["cases"][case] = {
        "packed_pinned_steady": summary(pin_p), "strided_pinned_steady": summary(pin_s),
        "packed_unpinned": summary(unp_p), "strided_unpinned": summary(unp_s),
        "packed_pinned_first_ms": round(first_p, 3), "strided_pinned_first_ms": round(first_s, 3),
        "strided_over_packed_pinned": round(ps / pp, 4), "pinned_alternating_spread": round(spread, 4),
        "strided_over_packed_unpinned": round(us / up, 4),
        "host_bytes_per_call_unpinned": {"packed": hb.nbytes + hs.nbytes, "strided": sb.data.nbytes + hs.nbytes},
        "same_result_every_call": len(res) == 1,
    }
    del hb, hs, sb

if a.pack_stats:
    rows = []
    for path in glob.glob(os.path.join(a.pack_stats, "**", "*kernel_stats.csv"), recursive=True):
        rows += [r for r in csv.DictReader(open(path)) if "records_pack" in r["Name"]]
    # bytes records_pack moved in the --pack-only run: n * (stride + packed record) per case (G1 72 + 64, G2 136 + 128)
    moved = {4: (2**20 + 2**26) * (72 + 64), 8: 2**20 * (136 + 128)}
    pack = {}
    for r in rows:
        pieces = 4 if "records_pack<4" in r["Name"] else 8
        ns = float(r["TotalDurationNs"])
        pack["G1" if pieces == 4 else "G2"] = {"kernel": r["Name"].split("(")[0], "calls": int(r["Calls"]), "total_ms": round(ns / 1e6, 3),
                                              "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "bytes": moved[pieces],
                                              "TB_per_s": round(moved[pieces] / ns / 1e3, 3)}
    out["records_pack"] = pack
print(json.dumps(out))
