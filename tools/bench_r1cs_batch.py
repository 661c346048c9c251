#!/usr/bin/env python3
"""B witnesses of one circuit: ONE batch product against the loop of B single products, and the satisfaction check
(profiles/r1cs_batch.md).

The synthetic circuit of tools/bench_r1cs_eval.py (its stated row-length and coefficient distribution) at 2^16 and 2^20 constraints,
B = 4 and 16 witnesses (the benchmark's witness, rotated by k variables for witness k).  Per (size, B), in ONE process and in alternation,
each behind --warm-ms of the same call, by device events over --iters calls:
  loop    B calls of mi355zk_bn254_fr_sparse_matvec_dev -- the path prove_many took before, still in the library
  batch   one call of mi355zk_bn254_fr_sparse_matvec_batch_dev (--ab-so name=path: the same call from further builds, another R1CS_BATCH_V)
after checking once that both leave the same bytes.  Then the wall time of mi355zk_bn254_fr_r1cs_check_dev over the batch (it ends in a
stream synchronise) and of circom.prepare_provers_dev against the loop of circom.prepare_prover_dev.  Medians and minima over --reps.
One JSON line per (size, B); `batch_not_above_loop` at B = 16, 2^16 is the condition prepare_provers_dev's one-launch path rests on."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", default="16,20")
    ap.add_argument("--batch", default="4,16")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm-ms", type=float, default=50.0)
    ap.add_argument("--ab-so", default="", help="comma-separated name=path of further library builds to time the batch call with")
    a = ap.parse_args()

    import torch

    import phase2_bn254_amd as zk
    from bench_r1cs_eval import synthetic_circuit

    assert torch.cuda.is_available(), "this benchmark measures the device: no GPU, no number"
    dev = torch.device("cuda", 0)
    lib = zk.lib.load()
    batch_libs = {"default": lib}
    for item in filter(None, a.ab_so.split(",")):
        name, path = item.split("=")
        other = C.CDLL(os.path.abspath(path))
        fn = other.mi355zk_bn254_fr_sparse_matvec_batch_dev
        fn.restype, fn.argtypes = zk.lib.SIGNATURES["mi355zk_bn254_fr_sparse_matvec_batch_dev"]
        batch_libs[name] = other
    sync = torch.cuda.synchronize
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731
    stats = lambda ts: {"median": round(float(np.median(ts)), 5), "min": round(float(min(ts)), 5), "max": round(float(max(ts)), 5)}  # noqa: E731

    t_start = time.perf_counter()
    for log_n in [int(v) for v in a.log_n.split(",")]:
        circuit, w = synthetic_circuit(zk, log_n)
        cc = zk.circom.compile_circuit(circuit, dev)
        print(f"2^{log_n}: circuit built and compiled {time.perf_counter() - t_start:.0f} s after the start", file=sys.stderr, flush=True)
        n_vars, rows = int(w.shape[0]), 3 * cc.m
        matrix = (ptr(cc.row_ptr), ptr(cc.col), ptr(cc.coeff_id), ptr(cc.coeffs), cc.n_coeffs)
        for n_batch in [int(v) for v in a.batch.split(",")]:
            ws = np.stack([np.roll(w, k, axis=0) for k in range(n_batch)])
            ws[:, 0] = (1, 0, 0, 0)
            d_w = torch.cat([torch.cat([p.input_assignment, p.aux_assignment]) for p in zk.circom.prepare_provers_dev(cc, ws)]).reshape(n_batch, n_vars, 4)
            out_loop = torch.zeros((n_batch, rows, 4), dtype=torch.int64, device=dev)
            out_batch = torch.zeros((n_batch, rows, 4), dtype=torch.int64, device=dev)

            def loop():
                for v in range(n_batch):
                    assert lib.mi355zk_bn254_fr_sparse_matvec_dev(ptr(out_loop[v]), *matrix, ptr(d_w[v]), n_vars, rows, cc.nnz, stream()) == 0

            def batch(which):
                assert which.mi355zk_bn254_fr_sparse_matvec_batch_dev(ptr(out_batch), rows, *matrix, ptr(d_w), n_vars, n_vars, n_batch, rows,
                                                                      cc.nnz, stream()) == 0

            calls = {"loop": loop}
            calls.update({f"batch[{name}]": (lambda which=which: batch(which)) for name, which in batch_libs.items()})
            loop()
            for name, which in batch_libs.items():                              # same bytes from the loop and from every build's batch call
                out_batch.zero_()
                batch(which)
                sync()
                assert torch.equal(out_batch, out_loop), name
            times = {name: [] for name in calls}
            for _ in range(a.reps):                                             # in alternation
                for name, fn in calls.items():
                    t_warm = time.perf_counter() + a.warm_ms * 1e-3
                    while time.perf_counter() < t_warm:                         # (a synchronise per call: one launch of milliseconds is enqueued
                        fn()                                                    # in microseconds, and an unbounded queue would be minutes of work)
                        sync()                                                  # the timed calls start on an idle queue
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.iters):
                        fn()
                    e1.record()
                    e1.synchronize()
                    times[name].append(e0.elapsed_time(e1) / a.iters)
            res = {"log_n": log_n, "n_batch": n_batch, "rows": rows, "nnz": cc.nnz, "n_vars": n_vars, "tile_V": zk.lib.R1CS_BATCH_V}
            for name, ts in times.items():
                res[f"{name}_ms"] = stats(ts)
            res["batch_not_above_loop"] = res["batch[default]_ms"]["median"] <= res["loop_ms"]["median"]

            first, count = (C.c_longlong * n_batch)(), (C.c_uint32 * n_batch)()

            def check():
                assert lib.mi355zk_bn254_fr_r1cs_check_dev(ptr(out_batch), C.c_void_p(out_batch.data_ptr() + 32 * cc.m),
                                                           C.c_void_p(out_batch.data_ptr() + 64 * cc.m), cc.m, rows, n_batch, first, count, stream()) == 0

            def wall(fn, reps):
                ts = []
                for _ in range(reps):
                    sync()
                    t = time.perf_counter()
                    fn()
                    sync()
                    ts.append(1e3 * (time.perf_counter() - t))
                return stats(ts)

            check()
            res["check_wall_ms"] = wall(check, a.reps * a.iters)
            res["check_failing_rows_of_witness_0"] = int(count[0])              # (the synthetic witness satisfies nothing in particular)
            zk.circom.prepare_provers_dev(cc, ws)
            res["prepare_provers_dev_wall_ms"] = wall(lambda: zk.circom.prepare_provers_dev(cc, ws), a.reps)
            res["prepare_prover_dev_loop_wall_ms"] = wall(lambda: [zk.circom.prepare_prover_dev(cc, ws[k]) for k in range(n_batch)], a.reps)
            res["elapsed_s"] = round(time.perf_counter() - t_start, 1)
            print(json.dumps(res), flush=True)
            del d_w, out_loop, out_batch
        del circuit, cc


if __name__ == "__main__":
    main()
