#!/usr/bin/env python3
"""The R1CS evaluation of a circom proof, compiled circuit against the Python restatement (profiles/r1cs_eval.md).

A synthetic circuit with a STATED length distribution: a domain of n = 2^log_n rows per matrix, of which the last n / 16 are the empty
padding rows (n - n / 16 - 16 constraints and the 16 input rows); every A, B and C combination has 1 .. 5 terms, uniformly (3 on average);
every 64th constraint's A combination is a 254-term bit decomposition (coefficients 2^0 .. 2^253 over consecutive variables), and every
16384th constraint's B combination has 4096 terms (the occasional row of thousands).  Coefficients otherwise: 1 (60 %), -1 (20 %),
a power of two (19 %), uniform (1 %).  n variables; witness values as in a Groth16 witness (tests/test_gpu_msm.py
test_prover_like_exponents_at_2e22_take_the_big_bin_path): 40 % ones, 30 % zeros, 10 % bytes, the rest uniform.

Per size: compile_circuit wall time; prepare_prover_dev wall time (array and list form of the witness; the witness upload alone); the
sparse product's time by device events behind --warm-ms of the same call, and its bytes/s over the algorithmic traffic -- per term 4 B
col + 4 B coeff_id + 32 B gathered x, per row 32 B written.  --with-python (2^16): the wall time of circom.prepare_prover on the same
circuit.  --ab-so: further builds of the library (another R1CS_SHORT_ROW_MAX), timed on the same device arrays in alternation.
One JSON line per size."""
import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402

R = 21888242871839275222246405745257275088548364400416034343698204186575808495617
HBM_ACHIEVABLE = 6.3e12   # B/s: VERDICT.md, from profiles/r06_partition_pmc.txt
NUM_INPUTS = 16


def synthetic_circuit(zk, log_n: int, seed: int = 7):
    rng = np.random.default_rng(seed)
    n = 1 << log_n
    n_c, n_vars = n - n // 16 - NUM_INPUTS, n
    pow2 = [1 << k for k in range(254)]
    lens = rng.integers(1, 6, size=(n_c, 3))
    total = int(lens.sum())
    cols = rng.integers(0, n_vars, size=total).tolist()
    kind = rng.random(total)
    shift = rng.integers(1, 254, size=total).tolist()
    wide = [int.from_bytes(rng.bytes(40), "little") % R for _ in range(int((kind >= 0.99).sum()))]
    wi = iter(wide)
    coeffs = [1 if k < 0.6 else R - 1 if k < 0.8 else pow2[s] if k < 0.99 else next(wi) for k, s in zip(kind.tolist(), shift)]
    constraints, t = [], 0
    starts = rng.integers(0, n_vars - 254, size=n_c // 64 + 1).tolist()
    for i, (la, lb, lc) in enumerate(lens.tolist()):
        a = list(zip(cols[t:t + la], coeffs[t:t + la])); t += la   # noqa: E702
        b = list(zip(cols[t:t + lb], coeffs[t:t + lb])); t += lb   # noqa: E702
        c = list(zip(cols[t:t + lc], coeffs[t:t + lc])); t += lc   # noqa: E702
        if i % 64 == 63:
            s = starts[i // 64]
            a = list(zip(range(s, s + 254), pow2))
        if i % 16384 == 16383:
            b = list(zip(rng.integers(0, n_vars, size=4096).tolist(), [1, R - 1] * 2048))
        constraints.append((a, b, c))
    kinds = rng.integers(0, 10, size=n_vars)
    w = np.zeros((n_vars, 4), dtype=np.uint64)
    w[kinds < 4, 0] = 1
    w[kinds == 7, 0] = rng.integers(0, 256, size=int((kinds == 7).sum()), dtype=np.uint64)
    uni = kinds >= 8
    w[uni] = rng.integers(0, 1 << 61, size=(int(uni.sum()), 4), dtype=np.uint64)   # (< 2^253 < r: canonical)
    w[0] = (1, 0, 0, 0)
    return zk.circom.CircomCircuit(NUM_INPUTS, n_vars - NUM_INPUTS, n_c, constraints), w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", default="16,20")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warm-ms", type=float, default=50.0)
    ap.add_argument("--with-python", default="16", help="sizes at which circom.prepare_prover is timed too")
    ap.add_argument("--ab-so", default="", help="comma-separated name=path of further library builds to time the product with")
    a = ap.parse_args()

    import torch

    import phase2_bn254_amd as zk

    assert torch.cuda.is_available(), "this benchmark measures the device: no GPU, no number"
    dev = torch.device("cuda", 0)
    libs = {"default": zk.lib.load()}
    for item in filter(None, a.ab_so.split(",")):
        name, path = item.split("=")
        lib = C.CDLL(os.path.abspath(path))
        fn = lib.mi355zk_bn254_fr_sparse_matvec_dev
        fn.restype, fn.argtypes = zk.lib.SIGNATURES["mi355zk_bn254_fr_sparse_matvec_dev"]
        libs[name] = lib
    sync = torch.cuda.synchronize
    ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)  # noqa: E731

    for log_n in [int(v) for v in a.log_n.split(",")]:
        t0 = time.perf_counter()
        circuit, w = synthetic_circuit(zk, log_n)
        t_build = time.perf_counter() - t0
        t0 = time.perf_counter()
        cc = zk.circom.compile_circuit(circuit, dev)
        sync()
        t_compile = time.perf_counter() - t0
        res = {"log_n": log_n, "rows": 3 * cc.m, "nnz": cc.nnz, "n_coeffs": cc.n_coeffs, "n_vars": int(w.shape[0]),
               "build_synthetic_s": round(t_build, 3), "compile_s": round(t_compile, 3)}

        def wall(fn):
            ts = []
            for _ in range(a.reps):
                sync()
                t = time.perf_counter()
                fn()
                sync()
                ts.append(time.perf_counter() - t)
            return round(1e3 * float(np.median(ts)), 4)

        zk.circom.prepare_prover_dev(cc, w)                                     # (first launches load the code objects)
        res["prepare_prover_dev_array_ms"] = wall(lambda: zk.circom.prepare_prover_dev(cc, w))
        res["witness_upload_ms"] = wall(lambda: torch.from_numpy(w.view(np.int64)).to(dev))
        w_ints = [int.from_bytes(row.tobytes(), "little") for row in w]
        res["prepare_prover_dev_list_ms"] = wall(lambda: zk.circom.prepare_prover_dev(cc, w_ints))

        pa = zk.circom.prepare_prover_dev(cc, w)
        d_w = torch.cat([pa.input_assignment, pa.aux_assignment]).contiguous()
        out = torch.empty((3 * cc.m, 4), dtype=torch.int64, device=dev)
        traffic = cc.nnz * (4 + 4 + 32) + 3 * cc.m * 32
        res["algorithmic_bytes"] = traffic

        def product(lib):
            rc = lib.mi355zk_bn254_fr_sparse_matvec_dev(ptr(out), ptr(cc.row_ptr), ptr(cc.col), ptr(cc.coeff_id), ptr(cc.coeffs), cc.n_coeffs, ptr(d_w),
                                                        int(w.shape[0]), 3 * cc.m, cc.nnz, stream())
            assert rc == 0

        kernel = {name: [] for name in libs}
        for name, lib in libs.items():                                          # same bytes from every build
            product(lib)
            sync()
            assert torch.equal(out[:cc.m], pa.a) and torch.equal(out[2 * cc.m:], pa.c), name
        for _ in range(a.reps):                                                 # the builds in alternation
            for name, lib in libs.items():
                t_warm = time.perf_counter() + a.warm_ms * 1e-3
                while time.perf_counter() < t_warm:
                    product(lib)
                sync()                                                          # (as tools/bench_ntt.py: the timed calls start on an idle queue)
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(a.iters):
                    product(lib)
                e1.record()
                e1.synchronize()
                kernel[name].append(e0.elapsed_time(e1) / a.iters)
        for name, ts in kernel.items():
            ms = float(np.median(ts))
            res[f"kernel_ms[{name}]"] = round(ms, 5)
            res[f"kernel_ms_min_max[{name}]"] = [round(min(ts), 5), round(max(ts), 5)]
            res[f"kernel_TBps[{name}]"] = round(traffic / (ms * 1e-3) / 1e12, 4)
            res[f"kernel_fraction_of_6.3TBps[{name}]"] = round(traffic / (ms * 1e-3) / HBM_ACHIEVABLE, 4)

        if str(log_n) in a.with_python.split(","):
            circuit.witness = w_ints
            t0 = time.perf_counter()
            ref = zk.circom.prepare_prover(circuit, dev)
            sync()
            res["prepare_prover_python_s"] = round(time.perf_counter() - t0, 3)
            n = cc.n
            assert torch.equal(ref.a, pa.a[:n]) and torch.equal(ref.b, pa.b[:n]) and torch.equal(ref.c, pa.c[:n])
        print(json.dumps(res), flush=True)
        del circuit, cc, pa, out, d_w


if __name__ == "__main__":
    main()
