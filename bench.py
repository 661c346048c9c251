#!/usr/bin/env python3
"""bench.py -- BASELINE.json's metric: BN254 G1 MSM throughput (Mscalar-mul/s) at 2^26 points.

  python bench.py [--gpus N] [--steps K] [--warmup W] [--log-n 26] [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

A plain run does only what the headline needs: input generation, W warm-up steps, the K timed steps, the dump of the
last step's result (--dump-outputs DIR: DIR/g1_msm_affine.npy, float64) and the JSON line with `value` and `ms_per_step`.
Everything else described below (the full-size linearity check, `roofline`, `cpu_baseline`, `value_incl_scalar_h2d`,
`secondary`, the N > 1 cross-checks and alternative plan) runs only with --full.

One "step" = one complete G1 multiexp over the whole 2^log_n-point input (bases and scalars already
resident in HBM): N ranks each run the single-GPU Pippenger on their contiguous point range
(SURVEY.md 8e), all-gather the 96-byte Jacobian partials over RCCL and add them on the host.
Total work is fixed as N grows ("scaling": "strong"), which is BASELINE.json config 4.
The input is the same for every N (generated in 2^LOG_SHARD-point shards seeded by the global
shard index), so the result of a step must be byte-identical across N; rank 0 checks the N-GPU result
against one more property each run: MSM(s) == MSM(s_even) + MSM(s_odd)-style split is exercised in
tests, here we check the partial-sum join against a second evaluation.

Adds to the JSON line: `roofline` (dominant kernel msm_accumulate, HBM model mandated by the
north-star plus the honest integer-ALU model) and `cpu_baseline` (oracle restatement of bellman's
multiexp timed on the host cores on a bounded sample); `value_incl_scalar_h2d` -- SURVEY 8(d)'s own
definition of the metric (one host-buffer call, bases on the device, the 2 GiB of exponents crossing
PCIe inside the timed region) next to `value` (everything resident, the bench contract's definition);
and, at N = 1, a `secondary` block: the other BASELINE configs (2^20 Fr NTT, 2^20 G1 / G2 multiexp,
phase2 contribute at 2^20), each with its own `roofline` and `cpu_baseline`, all timed in this run.
"""
from __future__ import annotations

import argparse
import contextlib
import ctypes as C
import gc
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

LOG_SHARD = 20  # input-generation granularity: identical total input for every N that divides 2^(log_n-LOG_SHARD)
R_TOP = 0x30644E72E131A029  # most-significant u64 limb of r
HBM_PEAK_GBS = 8000.0  # /opt/skills/guides/MI355X_MICROARCH.md: 8 TB/s spec
BYTES_PER_SCALAR_MUL = 96  # 64 B affine base + 32 B scalar, each read once
MADS_PER_MIXED_ADD = 1467  # curveu.hpp xyzzu_add_mixed: 7 u_mul (162) + 2 u_sqr (126) + 1 u_mul2 (243) v_mad_u64_u32
# integer-multiplier peak, MEASURED (tools/ubench_valu.hip, 4 waves/SIMD, independent chains): 28.3 T lane v_mad_u64_u32 / s on
# one MI355X (5.55 cycles per wave64 instruction per SIMD at the nominal 2.4 GHz; the 16-lane quarter-rate ideal would be 39.3 T)
MAD_PEAK_PER_S = 28.3e12


def gen_scalars(n: int, seed: int, device) -> torch.Tensor:
    """(n,4) int64 (bit pattern of u64 limbs): canonical FrRepr uniform in [0, r_top * 2^192) ~ [0, r)."""
    g = torch.Generator(device=device)
    g.manual_seed(seed)
    lo = torch.randint(0, 1 << 32, (n, 4), dtype=torch.int64, device=device, generator=g)
    hi = torch.randint(0, 1 << 32, (n, 3), dtype=torch.int64, device=device, generator=g)
    top = torch.randint(0, R_TOP >> 32, (n, 1), dtype=torch.int64, device=device, generator=g)
    hi = torch.cat([hi, top], dim=1)
    return (lo | (hi << 32)).contiguous()


def dump_outputs(path: str, L, result) -> None:
    """--dump-outputs: the group element the timed step hands its caller, as g1_msm_affine.npy (2, 8): x | y of the affine
    normalisation of the (12,) u64 Jacobian result (all-zero = infinity), each u64 as its two 32-bit words (low first) in
    float64, so every value is exact.  (The Jacobian coordinates themselves are not written: the point is the same from run
    to run, its projective representation is not.)"""
    os.makedirs(path, exist_ok=True)
    aff = np.zeros(8, dtype=np.uint64)
    rc = L.mi355zk_bn254_g1_to_affine(aff.ctypes.data_as(C.c_void_p), np.ascontiguousarray(result, dtype=np.uint64).ctypes.data_as(C.c_void_p))
    assert rc == 0, rc
    np.save(os.path.join(path, "g1_msm_affine.npy"), aff.astype("<u8").view("<u4").astype(np.float64).reshape(2, 8))


def kernel_sources_sha() -> str:
    """hash of the sources the dominant kernel is compiled from: ties a committed PMC figure to the code it was measured on"""
    import hashlib

    h = hashlib.sha256()
    for f in ("msm_impl.hpp", "curveu.hpp", "fieldu.hpp", "msm_g1.hip"):
        with open(os.path.join(ROOT, "phase2-bn254_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def ntt_sources_sha() -> str:
    """the same lock for the NTT pass's PMC figure (profiles/latest_pmc_ntt.json)"""
    import hashlib

    h = hashlib.sha256()
    for f in ("ntt.hip", "fieldu.hpp"):
        with open(os.path.join(ROOT, "phase2-bn254_amd", "csrc", f), "rb") as fh:
            h.update(fh.read())
    return h.hexdigest()[:16]


def host_cpu_info() -> dict:
    """what the cpu_baseline figures were timed on (the same '16 threads of a 256-core host' read 3.04 and 2.57 M/s on two boxes)"""
    info = {"logical_cpus": os.cpu_count()}
    try:
        with open("/proc/cpuinfo") as f:
            txt = f.read()
        models = [ln.split(":", 1)[1].strip() for ln in txt.splitlines() if ln.startswith("model name")]
        mhz = [float(ln.split(":", 1)[1]) for ln in txt.splitlines() if ln.startswith("cpu MHz")]
        info["model"] = models[0] if models else None
        info["sockets"] = len({ln.split(":", 1)[1].strip() for ln in txt.splitlines() if ln.startswith("physical id")}) or None
        info["cpu_mhz_now_min_max"] = [round(min(mhz)), round(max(mhz))] if mhz else None
    except OSError:
        pass
    try:
        with open("/sys/devices/system/cpu/cpu0/cpufreq/scaling_governor") as f:
            info["governor"] = f.read().strip()
    except OSError:
        info["governor"] = None
    try:
        info["loadavg_1m"] = round(os.getloadavg()[0], 2)
    except OSError:
        pass
    return info


def _ntt_traffic(log_n: int):
    """HBM bytes per ntt_pass_kernel launch from the committed PMC record, only while it was measured at this size on these sources"""
    try:
        with open(os.path.join(ROOT, "profiles", "latest_pmc_ntt.json")) as f:
            pmc = json.load(f)
        if pmc.get("workload_log_n") == log_n and pmc.get("kernel_sources_sha") == ntt_sources_sha():
            return pmc["hbm_bytes_per_launch"]
    except (OSError, ValueError, KeyError):
        pass
    return None


def _prof(L, names):
    res = {}
    for name in names:
        ms, cnt = C.c_double(), C.c_long()
        L.mi355zk_prof_get(name.encode(), C.byref(ms), C.byref(cnt))
        res[name] = (ms.value / cnt.value) if cnt.value else None
    return res


# The interpreter's cyclic garbage collector: with torch imported a full (generation-2) collection walks a few hundred thousand objects --
# tens of milliseconds -- and it fires wherever the allocation counters happen to trip.  BENCH_r04's "G1 table mode 3.24 ms" was 20 calls of
# 1.39 ms plus ONE such pause (round 5 reproduced it: ms_min_median_max = [3.69, 3.79, 38.2] in the G2 table leg of two driver-style runs,
# none in tools/diag_table_calls.py's 200 calls).  Every timed loop of the secondary legs therefore runs like `timeit` does: collect first,
# collector off inside.  The callback below logs each collection so the JSON line says what was seen (`host_gc`).
_GC_LOG = []


def _gc_cb(phase, info):
    if phase == "start":
        _gc_cb.t0 = time.perf_counter()
    else:
        _GC_LOG.append((int(info.get("generation", -1)), (time.perf_counter() - getattr(_gc_cb, "t0", time.perf_counter())) * 1e3))


gc.callbacks.append(_gc_cb)


@contextlib.contextmanager
def _no_gc(collect: bool = True):
    if collect:
        gc.collect()
    was = gc.isenabled()
    gc.disable()
    try:
        yield
    finally:
        if was:
            gc.enable()


def _timed(fn, iters, collect: bool = True):
    # (the collection -- tens of milliseconds with the GPU idle -- comes BEFORE the warm-up: a 0.12-ms transform timed right after it
    # runs on clocks that have dropped; the first refresh of round 5 read the NTT 8 % slow that way)
    with _no_gc(collect):
        fn()
        fn()
        torch.cuda.synchronize()
        t = time.perf_counter()
        for _ in range(iters):
            r = fn()
        torch.cuda.synchronize()
        dt = (time.perf_counter() - t) / iters
    return dt, r


def secondary(zk, L, worker, dev, log_n: int, cpu: bool = True) -> dict:
    """The other BASELINE.json configs on one MI355X, inputs resident in HBM, each with the roofline of its dominant kernel
    (algorithmic bytes of SURVEY 8d / HIP-event kernel time) and the oracle's restatement of the reference's CPU path timed on
    this host: config 3 (2^20 Fr NTT: fft / ifft / coset_fft; CPU serial_fft and the radix-P parallel_fft, domain.rs:274-376),
    config 2 (2^20 G1 multiexp; CPU in powersoftau's `dense` shape -- all cores on one region at a time, utils.rs:189-292 -- and
    bellman's one-thread-per-window shape), the G2 multiexp, and config 5 (phase2 contribute: L and H times delta^-1,
    parameters.rs:423-470; CPU: the oracle's wNAF-free mul_assign per point on a sample).  ~6 s in all."""
    import inputs
    import oracle_lib as O
    import bn254_model as M

    n = 1 << log_n
    cores = os.cpu_count() or 1
    sec = {}

    # ---- Fr NTT
    host = inputs.random_fr_mont(n, seed=5)
    d = torch.from_numpy(host.view(np.int64)).to(dev)
    ntt = {}
    pass_ms, passes, pass_ms_events_per_launch = None, None, None
    for op in ("fft", "ifft", "coset_fft"):
        dom = zk.EvaluationDomain(d.clone(), log_n)
        # Timed WITHOUT the library's per-kernel HIP events and after a warm-up: rounds 1-3 recorded two events per pass inside the
        # timed loop (~5 us each on a 60-us kernel) and timed `fft` first, on clocks that had just idled through the input
        # generation -- together 10-15 % on this 0.12-ms operation (tools/bench_ntt.py shows both effects).  The per-pass kernel time
        # for the roofline comes from a second, instrumented loop.
        gc.collect()
        t_warm = time.perf_counter() + 0.04   # (40 ms of back-to-back transforms: the collection above left the GPU idle for ~50 ms, and 40 calls
        while time.perf_counter() < t_warm:   #  = 5 ms did not bring the clocks back: ifft / coset_fft read 5-8 % slow behind it)
            getattr(dom, op)(worker)
        dt, _ = _timed(lambda: getattr(dom, op)(worker), 40, collect=False)
        ntt[op] = {"ms": round(dt * 1e3, 4), "Melem_per_s": round(n / dt / 1e6, 1)}
        if op == "fft":
            L.mi355zk_prof_reset()
            L.mi355zk_prof_enable(1)
            _timed(lambda: getattr(dom, op)(worker), 20)
            L.mi355zk_prof_enable(0)
            ms, cnt = C.c_double(), C.c_long()
            L.mi355zk_prof_get(b"ntt_pass", C.byref(ms), C.byref(cnt))
            if cnt.value:
                pass_ms, passes = ms.value / cnt.value, cnt.value / 21.0
            # (round 5) the library's per-pass events bracket EVERY launch: two event records around a 50-us kernel put ~6 us on it (61.9 us here
            # against 51.7 us per launch in rocprofv3's kernel trace, profiles/r05_final_ntt_pass_split.txt).  The figure the roofline uses
            # is one pair of HIP events on the stream the passes run on (torch's current stream) around 40 back-to-back transforms, divided by
            # their launches: the launch gaps (~2 us each) stay inside, the event overhead does not.
            if passes:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                with _no_gc(False):
                    t_warm = time.perf_counter() + 0.04   # (the instrumented loop above collected garbage first: clocks down again)
                    while time.perf_counter() < t_warm:
                        dom.fft(worker)
                    e0.record()
                    for _ in range(40):
                        dom.fft(worker)
                    e1.record()
                    e1.synchronize()
                pass_ms_events_per_launch, pass_ms = pass_ms, e0.elapsed_time(e1) / (40 * round(passes))
    # (round 5) the prover's shape (prover.rs:217-241): a, b and c through ifft and coset_fft -- three independent transforms per operation,
    # one launch per pass over all three (mi355zk_bn254_fr_domain_op_batch_dev); per transform
    doms3 = [zk.EvaluationDomain(d.clone(), log_n) for _ in range(3)]
    for op in ("ifft", "coset_fft"):
        fn = getattr(zk.EvaluationDomain, op + "_many")
        gc.collect()
        t_warm = time.perf_counter() + 0.04
        while time.perf_counter() < t_warm:
            fn(worker, doms3)
        dt3, _ = _timed(lambda: fn(worker, doms3), 20, collect=False)
        ntt[op]["ms_per_transform_in_a_batch_of_3"] = round(dt3 / 3 * 1e3, 4)
    del doms3
    achieved = 64 * n / (pass_ms * 1e-3) / 1e9 if pass_ms else None
    entry = {"metric": "2^%d-element BN254 Fr NTT (EvaluationDomain fft / ifft / coset_fft), in place in HBM" % log_n, **ntt,
             "roofline": {"bound": "hbm", "kernel": "ntt_pass_kernel", "achieved": round(achieved, 1) if achieved else None, "peak": HBM_PEAK_GBS,
                          "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4) if achieved else None,
                          # a SEPARATE rocprofv3 --pmc pass, hash-locked to ntt.hip + fieldu.hpp (profiles/latest_pmc_ntt.json): null rather than stale
                          "traffic": _ntt_traffic(log_n),
                          "passes_per_transform": round(passes) if passes else None, "pass_ms": round(pass_ms, 4) if pass_ms else None,
                          "pass_ms_with_an_event_pair_per_launch": round(pass_ms_events_per_launch, 4) if pass_ms_events_per_launch else None,
                          "note": "algorithmic 64 B per element per pass (32 B read + 32 B written); the pass is VALU-issue bound (DESIGN.md 3)"}}
    if cpu:
        omega = O.fr_domain(log_n)[0]
        t = time.perf_counter()
        want = O.fr_serial_fft(host, log_n, omega)
        dt_serial = time.perf_counter() - t
        log_cpus = min(int(np.log2(cores)), 6)
        t = time.perf_counter()
        par = O.fr_parallel_fft(host, log_n, omega, log_cpus)
        dt_par = time.perf_counter() - t
        dom = zk.EvaluationDomain(d.clone(), log_n)
        dom.fft(worker)
        ok = bool(np.array_equal(dom.coeffs.cpu().numpy().view(np.uint64).reshape(-1), want.reshape(-1)) and np.array_equal(par, want))
        # the reference itself uses log2(num_cpus) (multicore.rs:37-39), not a cap: the same transform once with every core of THIS host
        log_all = int(np.log2(cores))
        dt_all = None
        if log_all > log_cpus and log_all < log_n:
            t = time.perf_counter()
            par_all = O.fr_parallel_fft(host, log_n, omega, log_all)
            dt_all = time.perf_counter() - t
            assert np.array_equal(par_all, want)
        entry["cpu_baseline"] = {"value": round(n / dt_par / 1e6, 3), "unit": "Melem/s", "cores": 1 << log_cpus, "kind": "port",
                                 "uncapped": None if dt_all is None else {"cores": 1 << log_all, "Melem_per_s": round(n / dt_all / 1e6, 3),
                                                                        "note": "log_cpus = log2(num_cpus) as multicore.rs:37-39 computes it on this host"},
                                 "sample": "the same 2^%d elements, one fft: oracle restatement of bellman's parallel_fft (radix-%d first stage, "
                                           "domain.rs:319-376), %.3f s; serial_fft (domain.rs:274-317) on one core: %.3f s = %.3f Melem/s"
                                           % (log_n, 1 << log_cpus, dt_par, dt_serial, n / dt_serial / 1e6),
                                 "serial_fft_Melem_per_s": round(n / dt_serial / 1e6, 3), "gpu_matches_oracle": ok}
    sec["fr_ntt_2e%d" % log_n] = entry
    del d

    # ---- G1 / G2 multiexp
    for group, limbs, gen, name in ((1, 8, inputs.G1_GEN_RAW, "g1"), (2, 16, inputs.G2_GEN_RAW, "g2")):
        sc = gen_scalars(n, 11 + group, dev)
        k = gen_scalars(n, 21 + group, dev)
        b = torch.empty((n, limbs), dtype=torch.int64, device=dev)
        genr = np.ascontiguousarray(gen)
        fn = L.mi355zk_bn254_g1_batch_mul_dev if group == 1 else L.mi355zk_bn254_g2_batch_mul_dev
        assert fn(C.c_void_p(b.data_ptr()), genr.ctypes.data_as(C.c_void_p), C.c_void_p(k.data_ptr()), n, None) == 0
        # warm-up: the CPU baseline of the previous leg has just had every host core busy (its worker threads, numpy / torch pools that keep
        # spinning for a while after their last parallel region): a 2-ms call is ~27 kernel launches, and launches issued beside spinning
        # threads measured 0.2 ms per call slower with IDENTICAL kernel times (profiles/r04_final_bench_n1.json against bench_2e20.json)
        time.sleep(0.3)
        gc.collect()   # (before the warm-up, not between it and the timed loop: see _timed)
        for _ in range(25 if group == 1 else 12):
            zk.multiexp(worker, (b, 0), zk.FullDensity(), sc).wait()
        iters = 20 if group == 1 else 10
        plain_calls = []
        with _no_gc(collect=False):
            for _ in range(iters):
                t = time.perf_counter()
                res = zk.multiexp(worker, (b, 0), zk.FullDensity(), sc).wait()
                plain_calls.append(time.perf_counter() - t)
            dt = sum(plain_calls) / iters   # (no per-kernel events in the timed loop: ~20 event records are 1-2 % of a 2-ms call)
        L.mi355zk_prof_reset()
        L.mi355zk_prof_enable(1)
        for _ in range(5):
            zk.multiexp(worker, (b, 0), zk.FullDensity(), sc).wait()
        L.mi355zk_prof_enable(0)
        kern = _prof(L, ("msm_digits", "msm_sort", "msm_accumulate_heavy", "msm_accumulate", "msm_reduce"))
        bytes_per = 96 if group == 1 else 160   # affine base + 32-byte exponent, each read once
        acc_ms = kern["msm_accumulate"]
        achieved = bytes_per * n / (acc_ms * 1e-3) / 1e9 if acc_ms else None
        entry = {"metric": "2^%d-point BN254 %s multiexp, FullDensity, bases + exponents resident in HBM" % (log_n, name.upper()),
                 "value": round(n / dt / 1e6, 2), "unit": "Mscalar-mul/s", "ms": round(dt * 1e3, 3),
                 "ms_min_median_max": [round(sorted(plain_calls)[i] * 1e3, 3) for i in (0, iters // 2, iters - 1)],
                 "roofline": {"bound": "hbm", "kernel": "msm_accumulate_kernel", "achieved": round(achieved, 2) if achieved else None,
                              "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 5) if achieved else None, "traffic": None,
                              "kernel_ms": {kk: (round(v, 4) if v is not None else None) for kk, v in kern.items()},
                              "note": "integer-ALU bound (DESIGN.md 4); %d B per scalar-mul algorithmic" % bytes_per}}
        # the same call in TABLE MODE (include/mi355zk.h: a precomputed window table of the base vector, one bucket set for all
        # windows) -- for vectors that do not change between calls, like the Parameters a prover queries; same affine point
        tb = zk.MsmTable(b)
        torch.cuda.synchronize()
        gc.collect()
        for _ in range(25 if group == 1 else 12):      # the plain leg's warm-up
            zk.multiexp(worker, (tb, 0), zk.FullDensity(), sc).wait()
        calls = []
        with _no_gc(collect=False):
            for _ in range(iters):
                t = time.perf_counter()
                res_t = zk.multiexp(worker, (tb, 0), zk.FullDensity(), sc).wait()
                calls.append(time.perf_counter() - t)
        dt_t = sum(calls) / iters
        L.mi355zk_prof_reset()
        L.mi355zk_prof_enable(1)
        for _ in range(5):
            zk.multiexp(worker, (tb, 0), zk.FullDensity(), sc).wait()
        L.mi355zk_prof_enable(0)
        kern_t = _prof(L, ("msm_digits", "msm_sort", "msm_accumulate_heavy", "msm_accumulate", "msm_reduce"))
        Gt = O.G1 if group == 1 else O.G2
        entry["table_mode"] = {"value": round(n / dt_t / 1e6, 2), "unit": "Mscalar-mul/s", "ms": round(dt_t * 1e3, 3), "window_bits": tb.window_bits,
                               "windows": tb.n_windows, "table_MB": round(tb.table.numel() * 8 / 2**20, 1),
                               "ms_min_median_max": [round(sorted(calls)[i] * 1e3, 3) for i in (0, iters // 2, iters - 1)],
                               "kernel_ms": {kk: (round(v, 4) if v is not None else None) for kk, v in kern_t.items()},
                               "same_point": bool(np.array_equal(Gt.to_affine(res_t), Gt.to_affine(res)))}
        del tb
        if cpu:
            ns = n if group == 1 else n >> 2
            hb = b[:ns].cpu().numpy().view(np.uint64)
            hs = sc[:ns].cpu().numpy().view(np.uint64)
            G = O.G1 if group == 1 else O.G2
            cpus = min(cores, 64)
            t = time.perf_counter()
            dense = G.dense_multiexp(hb, hs, cpus=cpus)
            dt_dense = time.perf_counter() - t
            windows = (254 + O.multiexp_window_bits(ns) - 1) // O.multiexp_window_bits(ns)
            t = time.perf_counter()
            rc, sparse = G.multiexp(hb, hs, threads=min(cores, windows))
            dt_sparse = time.perf_counter() - t
            got = res if ns == n else zk.multiexp(worker, (b[:ns], 0), zk.FullDensity(), sc[:ns]).wait()
            ok = bool(rc == 0 and np.array_equal(G.to_affine(got), G.to_affine(dense)) and np.array_equal(G.to_affine(got), G.to_affine(sparse)))
            dt_dense_all = None
            if cores > cpus:   # powersoftau's dense_multiexp spreads a region over num_cpus::get() threads (utils.rs:216): once with all of them
                t = time.perf_counter()
                dense_all = G.dense_multiexp(hb, hs, cpus=cores)
                dt_dense_all = time.perf_counter() - t
                assert np.array_equal(G.to_affine(dense_all), G.to_affine(dense))
            entry["cpu_baseline"] = {"value": round(ns / dt_dense / 1e6, 4), "unit": "Mscalar-mul/s", "cores": cpus, "kind": "port",
                                     "uncapped": None if dt_dense_all is None else {"cores": cores, "Mscalar_mul_per_s": round(ns / dt_dense_all / 1e6, 4),
                                                                                  "note": "num_cpus threads per region, as utils.rs:216 takes them on this host"},
                                     "sample": "%s 2^%d points of the same input: oracle restatement of powersoftau dense_multiexp (all cores on one "
                                               "region at a time, utils.rs:189-292), %.2f s; bellman multiexp shape (one thread per window, %d "
                                               "threads): %.2f s = %.3f Mscalar-mul/s" % ("all" if ns == n else "the first", int(np.log2(ns)), dt_dense,
                                                                                        min(cores, windows), dt_sparse, ns / dt_sparse / 1e6),
                                     "bellman_shape_Mscalar_mul_per_s": round(ns / dt_sparse / 1e6, 4), "gpu_matches_oracle_on_sample": ok}
        sec["%s_msm_2e%d" % (name, log_n)] = entry
        del b, sc, k

    # ---- phase2 contribute (config 5): |L| = 2^log_n, |H| = 2^log_n - 1 G1 points times delta^-1, affine out
    k = gen_scalars(2 * n - 1, 901, dev)
    pts = torch.empty((2 * n - 1, 8), dtype=torch.int64, device=dev)
    genr = np.ascontiguousarray(inputs.G1_GEN_RAW)
    assert L.mi355zk_bn254_g1_batch_mul_dev(C.c_void_p(pts.data_ptr()), genr.ctypes.data_as(C.c_void_p), C.c_void_p(k.data_ptr()), 2 * n - 1, None) == 0
    delta = 0x0123456789ABCDEF0FEDCBA9876543210123456789ABCDEF % M.R_ORDER
    dinv_limbs = np.array([M.to_limbs(pow(delta, -1, M.R_ORDER))], dtype=np.uint64)
    dinv = torch.from_numpy(dinv_limbs.view(np.int64)).to(dev)
    l_before, h_before = pts[:n], pts[n:]

    def contribute():
        return zk.ceremony.batch_exp(l_before, dinv, same_scalar=True), zk.ceremony.batch_exp(h_before, dinv, same_scalar=True)

    dt, (l_after, h_after) = _timed(contribute, 3)
    npts = 2 * n - 1
    achieved = 128 * npts / dt / 1e9   # 64 B affine point read + 64 B affine point written
    entry = {"metric": "phase2 MPCParameters::contribute device work: |L| = 2^%d, |H| = 2^%d - 1 G1 points times delta^-1 (batch_exp), affine out"
                       % (log_n, log_n),
             "value": round(npts / dt / 1e6, 2), "unit": "Mpoint/s", "ms": round(dt * 1e3, 3),
             "roofline": {"bound": "hbm", "kernel": "batch_exp_kernel + batch_normalize_kernel", "achieved": round(achieved, 2), "peak": HBM_PEAK_GBS,
                          "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 6), "traffic": None,
                          "note": "128 B per point algorithmic; a 254-bit scalar multiplication per point: integer-ALU bound (DESIGN.md 4b); "
                                  "achieved is over the whole call (two kernels per vector)"}}
    if cpu:
        ns = 1 << 11
        hp = l_before[:ns].cpu().numpy().view(np.uint64)
        t = time.perf_counter()
        want = np.stack([O.G1.to_affine(O.G1.mul(O.G1.from_affine(hp[i]), dinv_limbs[0])) for i in range(ns)])
        dt_cpu = time.perf_counter() - t
        ok = bool(np.array_equal(l_after[:ns].cpu().numpy().view(np.uint64), want))
        entry["cpu_baseline"] = {"value": round(ns / dt_cpu / 1e6, 5), "unit": "Mpoint/s", "cores": 1, "kind": "port",
                                 "sample": "the first 2^11 points of L: oracle mul_assign + into_affine per point on one core (the reference spreads "
                                           "the same per-point work over its cores, parameters.rs:423-470), %.2f s" % dt_cpu,
                                 "gpu_matches_oracle_on_sample": ok}
    sec["contribute_2e%d" % log_n] = entry

    # ---- the single-process multi-GPU mode of the C ABI (mi355zk_init with n_devices > 1: include/mi355zk.h), only when this
    # process sees more than one GPU (the driver's N = 1 run on a multi-GPU node): ONE host thread calls mi355zk_bn254_g1_msm on host buffers
    # and the library cuts the call into one point range per device.  Run as a CHILD process (tools/bench_multi_device.py: 2^24 points,
    # pinned bases, page-locked exponents, upload inside the call) with a time limit: this mode has never run on real multi-GPU hardware,
    # and nothing it does may cost the headline line.
    phys = torch.cuda.device_count()
    ndev = int(os.environ.get("BENCH_MULTI_LOGICAL", phys))   # (test hook: k logical devices on the GPUs there are -- control flow, not scaling)
    if ndev > 1:
        import subprocess

        counts = [str(k) for k in (1, 2, 4, 8, 16) if k <= ndev]
        try:
            out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_multi_device.py"), "--log-n", "24", "--iters", "3", "--no-batch-exp", "--devices"] + counts,
                                 capture_output=True, text=True, timeout=240, cwd=ROOT)
            line = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
            sec["single_process_multi_gpu_2e24"] = json.loads(line[-1]) if out.returncode == 0 and line else {"error": "rc %d: %s" % (out.returncode, out.stderr[-300:])}
        except Exception as e:  # noqa: BLE001
            sec["single_process_multi_gpu_2e24"] = {"error": repr(e)[:300]}
    return sec


# ---- mad models of the scalar-multiplication kernels behind the "next" rows (api.hip; counts of v_mad_u64_u32 per lane, from the formulas'
# documented costs in curveu.hpp: Jacobian doubling 1071, table addition 2079, mixed addition 1593, U-form product 162)
# G1, per-point scalars (batch_exp_win_kernel<SPLIT>): GLV halves in 33 signed 4-bit windows: 128 doublings + 2 x 33 x 15/16 table additions
# (half of them with one more product by beta) + the {1..8}P table (4 doublings + 3 mixed additions)
MADS_G1_SCALAR_MUL = 128 * 1071 + 62 * 2079 + 31 * 162 + 4 * 1071 + 3 * 1593
# G2 default (plain windows, batch_exp_win_u2_kernel without the psi split): 65 windows = 260 doublings + 61 table additions + the table,
# every Fq2 product = 3 Fq products
MADS_G2_SCALAR_MUL_PLAIN = 3 * (260 * 1071 + 61 * 2079 + 4 * 1071 + 3 * 1593)
MADS_FQ2_MIXED_ADD = 3 * MADS_PER_MIXED_ADD
FQ_PRODUCT_PEAK_MEMORY_FORMAT = 125e9   # mont_mul_gfx950.inc: 125 G products/s (profiles/r05_final_ubench_fieldmul.txt)


def secondary_rows(zk, L, worker, dev, log_n: int, cpu: bool = True) -> dict:
    """SURVEY 8(f)'s rows on the same clock as the headline, inputs resident in HBM, every leg with the `roofline` of the
    call (algorithmic HBM bytes / call time, plus the multiplier-instruction model -- all of them are integer-ALU bound) and the oracle's
    restatement of the reference's loop timed on a bounded sample of the same input, compared record for record with the device's output:
      qap_eval      MPCParameters::new's per-variable sums (phase2/src/parameters.rs:225-294): CSR matrix x Lagrange points, G1 and G2 --
                    config 5's "G1 + G2 MSM mix"; general coefficients and circom-like ones (90 % +-1)
      power_pairs   powersoftau/src/utils.rs:112-135 (merge_pairs of v[..n-1], v[1..]: two multiexps over one random vector), G1 and G2
      point_ifft    prepare_phase2's Lagrange conversion (powersoftau/src/bin/prepare_phase2.rs:68-105; bellman/src/group.rs:22-51), G1
      decode        EncodedPoint::into_affine of a G1Compressed accumulator chunk (pairing/src/bn256/ec.rs:763-946)"""
    import inputs
    import oracle_lib as O
    import bn254_model as M

    n = 1 << log_n
    cores = os.cpu_count() or 1
    rows = {}
    vp = C.c_void_p
    r_minus_1 = torch.from_numpy(np.array(M.to_limbs(M.R_ORDER - 1), dtype=np.uint64).view(np.int64)).to(dev)
    one = torch.tensor([1, 0, 0, 0], dtype=torch.int64, device=dev)
    nw = C.c_int()
    L.mi355zk_msm_window_bits(n, C.byref(nw))
    for g, limbs, gen, name in ((1, 8, inputs.G1_GEN_RAW, "g1"), (2, 16, inputs.G2_GEN_RAW, "g2")):
        G = O.G1 if g == 1 else O.G2
        rec = 64 * g
        k = gen_scalars(n + 1, 31 + g, dev)
        bases = torch.empty((n + 1, limbs), dtype=torch.int64, device=dev)
        genr = np.ascontiguousarray(gen)
        mul = L.mi355zk_bn254_g1_batch_mul_dev if g == 1 else L.mi355zk_bn254_g2_batch_mul_dev
        assert mul(vp(bases.data_ptr()), genr.ctypes.data_as(vp), vp(k.data_ptr()), n + 1, None) == 0
        torch.cuda.synchronize()
        del k
        # -- QAP evaluation: n variables over n Lagrange points, 0..5 terms each, the constant ONE (variable 0) in n/4 terms
        g_ = torch.Generator(device=dev)
        g_.manual_seed(77 + g)
        lens = torch.randint(0, 6, (n,), device=dev, generator=g_, dtype=torch.int64)
        lens[0] = n // 4
        rp = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        rp[1:] = torch.cumsum(lens, 0)
        nnz = int(rp[-1].item())
        rp32 = rp.to(torch.int32)
        col = torch.randint(0, n, (nnz,), device=dev, generator=g_, dtype=torch.int32)
        cf = gen_scalars(nnz, 61 + g, dev)
        kind = torch.randint(0, 20, (nnz,), device=dev, generator=g_)
        cf_unit = cf.clone()
        cf_unit[kind < 9] = one
        cf_unit[(kind >= 9) & (kind < 18)] = r_minus_1
        out = torch.empty((n, limbs), dtype=torch.int64, device=dev)
        smv = L.mi355zk_bn254_g1_sparse_matvec_dev if g == 1 else L.mi355zk_bn254_g2_sparse_matvec_dev
        bytes_call = nnz * (rec + 32 + 4) + n * (rec + 4)
        mads_term = MADS_G1_SCALAR_MUL if g == 1 else MADS_G2_SCALAR_MUL_PLAIN
        entry = {"metric": "MPCParameters::new per-variable sums as one CSR x point-vector product (%s): %d rows, %d terms over 2^%d Lagrange points, affine out"
                           % (name.upper(), n, nnz, log_n), "rows": n, "terms": nnz}
        for label, coeffs in (("general_coefficients", cf), ("circom_like_90pct_unit_coefficients", cf_unit)):
            def call(c=coeffs):
                assert smv(vp(out.data_ptr()), vp(bases.data_ptr()), n, vp(rp32.data_ptr()), vp(col.data_ptr()), vp(c.data_ptr()), n, nnz, None, 0) == 0
            dt, _ = _timed(call, 2)
            general_terms = nnz if label.startswith("general") else int((kind >= 18).sum().item())
            entry[label] = {"ms": round(dt * 1e3, 2), "Mterm_per_s": round(nnz / dt / 1e6, 2),
                            "roofline": {"bound": "hbm", "kernel": "batch_exp_win%s_kernel + segsum" % ("" if g == 1 else "_u2"),
                                         "achieved": round(bytes_call / dt / 1e9, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                         "frac": round(bytes_call / dt / 1e9 / HBM_PEAK_GBS, 6), "traffic": None,
                                         "alu_model": {"mads_per_general_term": mads_term, "general_terms": general_terms,
                                                       "frac_of_mad_peak": round(general_terms * mads_term / dt / MAD_PEAK_PER_S, 4)},
                                         "note": "algorithmic bytes: %d B per term (base record + coefficient + column) + %d B per row; a scalar "
                                                 "multiplication per general term: integer-ALU bound%s" % (rec + 36, rec + 4, "" if g == 1 else
                                                 "; default flags: one subgroup-membership test per base, members' terms take the psi split "
                                                 "(fewer mads than the plain-window model: the fraction is an upper estimate)")}}
        if g == 2:
            def call_t():
                assert smv(vp(out.data_ptr()), vp(bases.data_ptr()), n, vp(rp32.data_ptr()), vp(col.data_ptr()), vp(cf.data_ptr()), n, nnz, None,
                           zk.lib.G2_TRUSTED_SUBGROUP) == 0
            dt, _ = _timed(call_t, 2)
            entry["general_coefficients_trusted_subgroup"] = {"ms": round(dt * 1e3, 2), "Mterm_per_s": round(nnz / dt / 1e6, 2)}
        if cpu:
            smv(vp(out.data_ptr()), vp(bases.data_ptr()), n, vp(rp32.data_ptr()), vp(col.data_ptr()), vp(cf.data_ptr()), n, nnz, None, 0)
            ns = 384 if g == 1 else 128
            h_rp = rp[1:ns + 2].cpu().numpy()     # rows 1 .. ns (row 0 is the n/4-term constant)
            t0, t1 = int(h_rp[0]), int(h_rp[-1])
            hb = bases[col[t0:t1].long()].cpu().numpy().view(np.uint64)
            hc = cf[t0:t1].cpu().numpy().view(np.uint64)
            t = time.perf_counter()
            want = np.zeros((ns, limbs), dtype=np.uint64)
            for r_ in range(ns):
                acc = G.from_affine(np.zeros(limbs, np.uint64))
                for j in range(int(h_rp[r_]) - t0, int(h_rp[r_ + 1]) - t0):
                    acc = G.add(acc, G.mul(G.from_affine(hb[j]), hc[j]))
                want[r_] = G.to_affine(acc)
            dt_cpu = time.perf_counter() - t
            entry["cpu_baseline"] = {"value": round((t1 - t0) / dt_cpu / 1e6, 5), "unit": "Mterm/s", "cores": 1, "kind": "port",
                                     "sample": "rows 1 .. %d of the same matrix (%d general terms): the oracle's mul_assign + add_assign per term and "
                                               "into_affine per row on one core (the reference spreads the variables over its cores, "
                                               "parameters.rs:250-294), %.2f s" % (ns, t1 - t0, dt_cpu),
                                     "gpu_matches_oracle_on_sample": bool(np.array_equal(out[1:ns + 1].cpu().numpy().view(np.uint64), want))}
        rows["qap_eval_%s_2e%d" % (name, log_n)] = entry
        del cf, cf_unit, col, kind, out, lens, rp, rp32

        # -- power_pairs: s = sum rho_i v_i, sx = sum rho_i v_{i+1} (two multiexps sharing digits and sorts)
        rho = gen_scalars(n, 41 + g, dev)
        mp = L.mi355zk_bn254_g1_merge_pairs_dev if g == 1 else L.mi355zk_bn254_g2_merge_pairs_dev
        s, sx = np.zeros(12 * g, np.uint64), np.zeros(12 * g, np.uint64)

        def pairs(m=n):
            assert mp(vp(bases.data_ptr()), vp(bases.data_ptr() + rec), vp(rho.data_ptr()), m, None, s.ctypes.data_as(vp), sx.ctypes.data_as(vp)) == 0
        for _ in range(3):
            pairs()
        dt, _ = _timed(pairs, 5)
        bytes_call = n * (rec + 32)
        mads = 2 * nw.value * n * (MADS_PER_MIXED_ADD if g == 1 else MADS_FQ2_MIXED_ADD)
        entry = {"metric": "powersoftau power_pairs over 2^%d + 1 %s points (merge_pairs(v[..n], v[1..]): both sums of one call)" % (log_n, name.upper()),
                 "ms": round(dt * 1e3, 3), "value": round(2 * n / dt / 1e6, 2), "unit": "Mscalar-mul/s (both sums)",
                 "roofline": {"bound": "hbm", "kernel": "msm_accumulate_kernel (two base vectors per digit)", "achieved": round(bytes_call / dt / 1e9, 2),
                              "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(bytes_call / dt / 1e9 / HBM_PEAK_GBS, 6), "traffic": None,
                              "alu_model": {"mads": mads, "frac_of_mad_peak": round(mads / dt / MAD_PEAK_PER_S, 4),
                                            "note": "%d windows x 2 sums x one mixed addition per point over the WHOLE call (digits, partition and the two "
                                                    "bucket reductions included in the time)" % nw.value},
                              "note": "algorithmic bytes: every point (v2 is v1 shifted by one record) and every rho_i once = %d B per point" % (rec + 32)}}
        if cpu:
            ns = 1 << 16
            pairs(ns)
            got_s, got_sx = G.to_affine(s.copy()), G.to_affine(sx.copy())
            hv = bases[:ns + 1].cpu().numpy().view(np.uint64)
            hr = rho[:ns].cpu().numpy().view(np.uint64)
            cpus = min(cores, 64)
            t = time.perf_counter()
            w_s, w_sx = G.dense_multiexp(hv[:ns], hr, cpus=cpus), G.dense_multiexp(hv[1:], hr, cpus=cpus)
            dt_cpu = time.perf_counter() - t
            entry["cpu_baseline"] = {"value": round(2 * ns / dt_cpu / 1e6, 4), "unit": "Mscalar-mul/s (both sums)", "cores": cpus, "kind": "port",
                                     "sample": "the first 2^16 + 1 points: the oracle's restatement of powersoftau dense_multiexp (utils.rs:189-292) for "
                                               "s and for sx, %d threads per region, %.2f s" % (cpus, dt_cpu),
                                     "gpu_matches_oracle_on_sample": bool(np.array_equal(got_s, G.to_affine(w_s)) and np.array_equal(got_sx, G.to_affine(w_sx)))}
        rows["power_pairs_%s_2e%d" % (name, log_n)] = entry
        del rho

        if g == 1:
            # -- G1 point ifft at 2^(log_n - 2) and compressed decode at 2^log_n
            ln = log_n - 2
            m = 1 << ln
            pts = bases[:m].clone()
            pf = L.mi355zk_bn254_g1_point_fft_dev
            assert pf(vp(pts.data_ptr()), ln, 1, None) == 0      # (warm-up; the transform of points is again a vector of points)
            torch.cuda.synchronize()
            with _no_gc():
                t = time.perf_counter()
                for _ in range(2):
                    assert pf(vp(pts.data_ptr()), ln, 1, None) == 0
                dt = (time.perf_counter() - t) / 2
            bfly = m // 2 * ln
            bytes_call = 128 * m * ln
            entry = {"metric": "EvaluationDomain<Point<G1>>::ifft over 2^%d points (prepare_phase2's Lagrange conversion), affine in and out" % ln,
                     "ms": round(dt * 1e3, 2), "value": round(bfly / dt / 1e6, 2), "unit": "Mbutterfly/s",
                     "roofline": {"bound": "hbm", "kernel": "pfft_stage_kernel", "achieved": round(bytes_call / dt / 1e9, 2), "peak": HBM_PEAK_GBS,
                                  "unit": "GB/s", "frac": round(bytes_call / dt / 1e9 / HBM_PEAK_GBS, 6), "traffic": None,
                                  "alu_model": {"mads_per_butterfly": MADS_G1_SCALAR_MUL + 2 * 2079, "frac_of_mad_peak":
                                                round(bfly * (MADS_G1_SCALAR_MUL + 2 * 2079) / dt / MAD_PEAK_PER_S, 4)},
                                  "note": "algorithmic bytes as the reference's serial_fft moves them: every stage reads and writes every point (128 B "
                                          "x n x log n); a butterfly is a scalar multiplication by the twiddle + an addition + a subtraction: integer-ALU bound"}}
            if cpu:
                ls = 9
                hp = bases[:1 << ls].cpu().numpy().view(np.uint64)
                t = time.perf_counter()
                want = O.point_domain_op(1, hp, ls, "ifft")
                dt_cpu = time.perf_counter() - t
                small = bases[:1 << ls].clone()
                assert pf(vp(small.data_ptr()), ls, 1, None) == 0
                entry["cpu_baseline"] = {"value": round((1 << ls) // 2 * ls / dt_cpu / 1e6, 5), "unit": "Mbutterfly/s", "cores": 1, "kind": "port",
                                         "sample": "the first 2^%d points: the oracle's Point<G1> serial_fft + batch_normalization (group.rs:22-51 under "
                                                   "domain.rs:274-317) on one core, %.2f s" % (ls, dt_cpu),
                                         "gpu_matches_oracle_on_sample": bool(np.array_equal(small.cpu().numpy().view(np.uint64), want))}
            rows["point_ifft_g1_2e%d" % ln] = entry
            del pts
            enc = torch.zeros((n, 32), dtype=torch.uint8, device=dev)
            back = torch.zeros((n, 8), dtype=torch.int64, device=dev)
            assert L.mi355zk_bn254_g1_encode_dev(vp(enc.data_ptr()), vp(bases.data_ptr()), n, 1, None) == 0

            def dec():
                assert L.mi355zk_bn254_g1_decode_dev(vp(back.data_ptr()), vp(enc.data_ptr()), n, 1, 1, None, None) == 0
            dt, _ = _timed(dec, 5)
            products = 252 + 127 + 6     # y = (x^3 + 3)^((q + 1) / 4) by square-and-multiply (field.hpp pow_limbs), x^3, the root test, the form changes
            entry = {"metric": "G1Compressed -> affine (EncodedPoint::into_affine, checked) of 2^%d points" % log_n, "ms": round(dt * 1e3, 3),
                     "value": round(n / dt / 1e6, 1), "unit": "Mpoint/s", "roundtrip_ok": bool(torch.equal(back, bases[:n])),
                     "roofline": {"bound": "hbm", "kernel": "g1_decode_kernel", "achieved": round(96 * n / dt / 1e9, 2), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                  "frac": round(96 * n / dt / 1e9 / HBM_PEAK_GBS, 6), "traffic": None,
                                  "alu_model": {"fq_products_per_point": products, "products_per_s": round(products * n / dt),
                                                "peak_products_per_s": FQ_PRODUCT_PEAK_MEMORY_FORMAT,
                                                "frac": round(products * n / dt / FQ_PRODUCT_PEAK_MEMORY_FORMAT, 4)},
                                  "note": "algorithmic bytes: 32 B in + 64 B out per point; one square root (a 252-bit power) per point: integer-ALU bound"}}
            if cpu:
                ns = 1 << 13
                henc = enc[:ns].cpu().numpy()
                t = time.perf_counter()
                rc_cpu, _, want = O.decode_points(1, henc, True, True)
                dt_cpu = time.perf_counter() - t
                assert rc_cpu == 0
                entry["cpu_baseline"] = {"value": round(ns / dt_cpu / 1e6, 5), "unit": "Mpoint/s", "cores": 1, "kind": "port",
                                         "sample": "the first 2^13 records: the oracle's restatement of G1Compressed::into_affine (ec.rs:763-946) on one core, "
                                                   "%.2f s" % dt_cpu,
                                         "gpu_matches_oracle_on_sample": bool(np.array_equal(back[:ns].cpu().numpy().view(np.uint64).reshape(-1),
                                                                                              np.asarray(want).reshape(-1)))}
            rows["decode_g1_compressed_2e%d" % log_n] = entry
            del enc, back
        del bases
    return rows


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--log-n", type=int, default=26)
    ap.add_argument("--cpu-sample-log-n", type=int, default=22)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--bases", choices=["random", "tau"], default="random",
                    help="random: P_i = k_i*G with independent k_i;  tau: the tau-table structure P_i = tau^i*G of the real workload (SURVEY 8d)")
    ap.add_argument("--no-h2d-leg", action="store_true", help="skip the extra timing that includes the scalars' host-to-device copy")
    ap.add_argument("--no-secondary", action="store_true", help="skip the secondary configs (NTT 2^20, G1 / G2 multiexp 2^20, contribute 2^20)")
    ap.add_argument("--secondary-log-n", type=int, default=20)
    ap.add_argument("--no-rows", action="store_true", help="skip the SURVEY 8(f) legs of the secondary block (QAP sums, power_pairs, point ifft, decode)")
    ap.add_argument("--full", action="store_true",
                    help="also run everything beyond the headline: per-kernel timings and roofline, the full-size linearity check, the N > 1 "
                         "cross-checks and alternative plan, the h2d leg, cpu_baseline and the secondary block (each --no-* flag still applies)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write the last step's G1 result (affine) to DIR/g1_msm_affine.npy (float64, exact 32-bit words)")
    args = ap.parse_args()

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if not torch.cuda.is_available():
        print("bench.py: no GPU visible (the product path has no CPU fallback)", file=sys.stderr)
        return 2
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        # `python bench.py --gpus N` as typed: launch the N ranks ourselves, exactly the way the driver's torchrun form does (one
        # process per GPU, RCCL), on a free port; the ranks' output is ours (rank 0 prints the one JSON line)
        import socket
        import subprocess

        ndev = torch.cuda.device_count()
        if os.environ.get("BENCH_BACKEND", "nccl") == "nccl" and ndev < args.gpus:
            print("bench.py: --gpus %d but %d GPU(s) visible (BENCH_BACKEND=gloo lets ranks share devices: control flow only, not a "
                  "scaling number)" % (args.gpus, ndev), file=sys.stderr)
            return 2
        with socket.socket() as sk:
            sk.bind(("127.0.0.1", 0))
            port = sk.getsockname()[1]
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
               "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
        return subprocess.call(cmd)
    if world != args.gpus:
        print("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world), file=sys.stderr)
        return 2
    # one process per GPU.  BENCH_BACKEND=gloo lets the N>1 control flow be exercised on a box with fewer
    # GPUs than ranks (ranks then share devices); the driver's multi-GPU run uses nccl (= RCCL over xGMI).
    backend = os.environ.get("BENCH_BACKEND", "nccl")
    ndev = torch.cuda.device_count()
    dev_index = local_rank if backend == "nccl" else local_rank % ndev
    torch.cuda.set_device(dev_index)
    dev = torch.device("cuda", dev_index)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev)
        else:
            dist.init_process_group(backend)

    import phase2_bn254_amd as zk
    import inputs

    L = zk.lib.load()
    worker = zk.Worker(dev_index)

    # ---- preflight (N > 1), BEFORE the input generation: the collective this run depends on, once, through the very code path the timed
    # steps use (shard._allgather_words: pinned -> H2D -> all_gather_into_tensor -> D2H on RCCL, the plain tensor form on gloo), with the
    # 14-word record of shard.exchange (12 Jacobian limbs + rc + index = 112 bytes).  A first lease of a real multi-GPU node then fails in
    # seconds with a message -- a missing IPC mode, a rank on the wrong device, a world that is not --gpus -- instead of after 40 s of setup.
    preflight = None
    if world > 1:
        t_pf = time.perf_counter()
        assert dist.get_world_size() == args.gpus, "torch.distributed sees %d ranks, --gpus %d" % (dist.get_world_size(), args.gpus)
        probe = np.arange(14, dtype=np.uint64) + (np.uint64(rank) << np.uint64(32))
        try:
            uuid = str(getattr(torch.cuda.get_device_properties(dev_index), "uuid", dev_index))
        except Exception:  # noqa: BLE001
            uuid = str(dev_index)
        probe[13] = np.uint64(int.from_bytes(__import__("hashlib").sha256(uuid.encode()).digest()[:7], "little"))
        got = zk.shard._allgather_words(probe, dev if backend == "nccl" else None, None, world)
        bad = [r for r in range(world) if got.shape != (world, 14) or int(got[r, 0]) != (r << 32) or int(got[r, 12]) != (r << 32) + 12]
        if bad:
            print("bench.py preflight: the 112-byte all-gather returned a wrong record for rank(s) %s" % bad, file=sys.stderr)
            return 3
        distinct = len({int(got[r, 13]) for r in range(world)})
        if backend == "nccl" and distinct != world:
            print("bench.py preflight: %d ranks on %d distinct GPU(s) (LOCAL_RANK -> device mapping)" % (world, distinct), file=sys.stderr)
            return 3
        preflight = {"ms": round((time.perf_counter() - t_pf) * 1e3, 1), "ranks": world, "distinct_devices": distinct, "record_bytes": 112,
                     "path": "shard._allgather_words (%s)" % ("pinned -> H2D -> all_gather_into_tensor -> D2H, one stream sync" if backend == "nccl" else "gloo, host tensors")}

    log_n = args.log_n
    n_total = 1 << log_n
    # sharding (shard.plan): a few contiguous point ranges x groups of scalar windows; BENCH_SHARD=points forces point ranges only
    if os.environ.get("BENCH_SHARD", "") == "points":
        pgroups, pgroup, wgroups, wgroup = world, rank, 1, 0
    else:
        pgroups, pgroup, wgroups, wgroup = zk.shard.rank_groups(world, rank)
    assert n_total % pgroups == 0
    n_local = n_total // pgroups
    shard = min(1 << LOG_SHARD, n_local)
    shards_local = n_local // shard
    first_shard = pgroup * shards_local

    # ---- synthetic inputs, generated on the device (no reference files): bases P_i = k_i * G
    scalars = torch.empty((n_local, 4), dtype=torch.int64, device=dev)
    bases = torch.empty((n_local, 8), dtype=torch.int64, device=dev)
    gen = np.ascontiguousarray(inputs.G1_GEN_RAW)
    t_gen = time.time()
    R_ORDER = 21888242871839275222246405745257275088548364400416034343698204186575808495617
    TAU = 0x2545F4914F6CDD1D9E3779B97F4A7C15F39CC0605CEDC8341082276BF3A27251 % R_ORDER
    for s in range(shards_local):
        gs = first_shard + s
        scalars[s * shard:(s + 1) * shard] = gen_scalars(shard, 1_000_003 * gs + 17, dev)
        if args.bases == "tau":   # P_i = tau^i * G for the GLOBAL index i (identical input for every N)
            k = zk.ceremony.scalar_powers(TAU, shard, dev, coeff=pow(TAU, gs * shard, R_ORDER))
        else:
            k = gen_scalars(shard, 2_000_003 * gs + 29, dev)
        rc = L.mi355zk_bn254_g1_batch_mul_dev(C.c_void_p(bases[s * shard:(s + 1) * shard].data_ptr()), gen.ctypes.data_as(C.c_void_p),
                                              C.c_void_p(k.data_ptr()), shard, C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
        torch.cuda.synchronize()
        del k
    t_gen = time.time() - t_gen
    lo_global = pgroup * n_local  # global index of this rank's first exponent

    def step(sc=None) -> np.ndarray:
        fut = zk.multiexp(worker, (bases, 0), zk.FullDensity(), scalars if sc is None else sc, window_group=(wgroups, wgroup))
        if world == 1:
            return fut.wait()  # (12,) u64 Jacobian
        # the path's one exchange step: all-gather of the 96-byte partials (+ rc and error index, so that a failing rank
        # cannot leave the others in the collective), then local EC adds
        return zk.shard.exchange(fut, 12, index_offset=lo_global, device=dev if backend == "nccl" else None)

    for _ in range(args.warmup):
        step()
    # Short steps (a 2^20 multiexp is 1.7 ms) are measured on a machine that has not reached its steady state after W = 1 warm-up: the
    # first ~10 calls of a process run on ramping clocks and cold host paths (same box: 1.99 ms after 1 warm-up step, 1.77 after 3, 1.675
    # after 50).  Steps shorter than 20 ms therefore get extra UNTIMED settle steps worth 0.2 s (reported as "settle_steps");
    # the 2^26 headline (67 ms per step) gets none.
    settle_steps = 0
    gc.collect()
    if args.warmup > 0 or args.steps > 0:
        t_probe = time.perf_counter()
        step()
        torch.cuda.synchronize()
        probe = time.perf_counter() - t_probe
        if world > 1:   # every rank must run the same number of steps (a step holds a collective): agree on the slowest probe
            tp = torch.tensor([probe], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
            dist.all_reduce(tp, op=dist.ReduceOp.MAX)
            probe = float(tp.item())
        settle_steps = 1
        if probe < 0.020:
            extra = min(400, int(0.2 / max(probe, 1e-5)))
            for _ in range(extra):
                step()
            settle_steps += extra

    # Inside the timed region only the DOMINANT kernel is bracketed by HIP events (two records per step, on the launch stream): the
    # roofline's `achieved` is measured live over exactly the timed steps.  The other kernel groups are timed in the linearity check's
    # launches below (same shape as a timed step): bracketing all eight groups costs ~20 event records = 0.1-0.2 ms of host time per
    # step -- nothing at 2^26, 10 % of a 2^20 step.  (--full only: a plain run times the steps without any event.)
    if args.full:
        L.mi355zk_prof_reset()
        L.mi355zk_prof_only(b"msm_accumulate")
        L.mi355zk_prof_enable(2 if world == 1 else 1)   # (a sharded step is a cell: the check's unsharded launches have another shape, so every group is timed here)
    if world > 1:
        dist.barrier()
    torch.cuda.synchronize()
    result = None
    with _no_gc(collect=False):   # (the interpreter's collector off inside the timed region, as `timeit` runs: see _GC_LOG; collected before the warm-up)
        t0 = time.perf_counter()
        for _ in range(args.steps):
            result = step()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        elapsed = time.perf_counter() - t0
    if args.full:
        L.mi355zk_prof_enable(0)
        acc_ms_timed, acc_cnt = C.c_double(), C.c_long()
        L.mi355zk_prof_get(b"msm_accumulate", C.byref(acc_ms_timed), C.byref(acc_cnt))
        acc_timed = (acc_ms_timed.value / acc_cnt.value) if acc_cnt.value else None
        if world == 1:
            L.mi355zk_prof_reset()
            L.mi355zk_prof_enable(1)   # (the check's launches below carry the per-group timings)
    if world > 1:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    if args.dump_outputs and rank == 0:
        dump_outputs(args.dump_outputs, L, result)

    additive_ok = sharded_ok = None
    if args.full:
        # size-independent check at the FULL size (outside the timed region): linearity in the exponents,
        #   MSM(bases, s) == MSM(bases, a) + MSM(bases, s - a)   with a uniform, s - a reduced mod r on the device.
        # (Every launch of the check has the shape of a timed step, so the per-kernel averages of a rocprofv3 trace of
        # this command are averages over identical launches.)
        sa = torch.empty_like(scalars)
        for s in range(shards_local):
            sa[s * shard:(s + 1) * shard] = gen_scalars(shard, 3_000_017 * (first_shard + s) + 41, dev)
        sb = scalars.clone()
        rc = L.mi355zk_bn254_fr_sub_assign_dev(C.c_void_p(sb.data_ptr()), C.c_void_p(sa.data_ptr()), n_local, None)
        assert rc == 0, rc
        torch.cuda.synchronize()
        # (over ALL windows of the local points: the partial over a window group is not linear in the exponents, the carries of
        # the signed digits cross windows)
        whole = result if world == 1 else zk.multiexp(worker, (bases, 0), zk.FullDensity(), scalars).wait()
        sharded_ok = True
        if world > 1:
            # the TIMED, sharded `result` itself (window-group partials -> all-gather -> join) against the unsharded evaluation:
            # one rank of every point range contributes `whole` (all windows of its points), the others the identity
            contrib = np.ascontiguousarray(whole) if wgroup == 0 else np.zeros(12, dtype=np.uint64)
            ref_total = zk.shard.allgather_join(contrib, device=dev if backend == "nccl" else None)
            ra, rb = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
            L.mi355zk_bn254_g1_to_affine(ra.ctypes.data_as(C.c_void_p), np.ascontiguousarray(ref_total).ctypes.data_as(C.c_void_p))
            L.mi355zk_bn254_g1_to_affine(rb.ctypes.data_as(C.c_void_p), np.ascontiguousarray(result).ctypes.data_as(C.c_void_p))
            sharded_ok = bool(np.array_equal(ra, rb))
            assert sharded_ok, "the sharded result differs from the unsharded evaluation"
        part_a = zk.multiexp(worker, (bases, 0), zk.FullDensity(), sa).wait()
        part_b = zk.multiexp(worker, (bases, 0), zk.FullDensity(), sb).wait()
        del sa, sb
        aff_a, aff_b = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
        L.mi355zk_bn254_g1_to_affine(aff_a.ctypes.data_as(C.c_void_p), np.ascontiguousarray(whole).ctypes.data_as(C.c_void_p))
        joined = zk.shard.join_partials(np.stack([part_a, part_b]))
        L.mi355zk_bn254_g1_to_affine(aff_b.ctypes.data_as(C.c_void_p), joined.ctypes.data_as(C.c_void_p))
        additive_ok = bool(np.array_equal(aff_a, aff_b))
        assert additive_ok, "full-size linearity check failed"

        # per-kernel durations measured with HIP events on the launch stream (library hooks): the dominant kernel over the timed steps,
        # the other groups over the check's launches (identical shapes)
        L.mi355zk_prof_enable(0)
        kern = {}
        for name in ("msm_digits", "msm_sort", "msm_part_scan", "msm_scatter", "msm_bucket", "msm_accumulate_heavy", "msm_accumulate", "msm_reduce"):
            ms, cnt = C.c_double(), C.c_long()
            L.mi355zk_prof_get(name.encode(), C.byref(ms), C.byref(cnt))
            kern[name] = (ms.value / cnt.value) if cnt.value else None
        if acc_timed is not None:
            kern["msm_accumulate"] = acc_timed

        # HBM traffic of the dominant kernel comes from a SEPARATE rocprofv3 --pmc pass (counters cannot be read from inside
        # this process): the committed figure is reported only when it was taken on this workload AND on these kernel sources
        # (profiles/latest_pmc.json records their hash) -- otherwise null, never a stale number.
        traffic = None
        try:
            with open(os.path.join(ROOT, "profiles", "latest_pmc.json")) as f:
                pmc = json.load(f)
            if pmc.get("workload_log_n") == log_n and pmc.get("n_gpus") == world and pmc.get("kernel_sources_sha") == kernel_sources_sha():
                traffic = pmc["hbm_bytes_per_launch"]
        except (OSError, ValueError, KeyError):
            pass

    # ---- (N > 1) the OTHER plan in the same run, so that the first real scaling record explains its own efficiency: the default plan gives a
    # rank a (point range x window group) cell (shard.plan: 1 x 2, 1 x 4, 2 x 4); the alternative is point ranges only (N x 1) -- every window
    # reduced once per rank, 1 / N of the points each.  Rank r's N x 1 range is the (r mod window_groups)-th part of the range it already
    # holds, so nothing is generated again.  Same barriers, same max-over-ranks clock, result checked against the timed plan's.
    alt_plan = None
    if args.full and world > 1 and wgroups > 1 and os.environ.get("BENCH_NO_ALT_PLAN") is None:
        n_alt = n_total // world
        off = wgroup * n_alt
        b_alt, s_alt = bases[off:off + n_alt], scalars[off:off + n_alt]
        lo_alt = lo_global + off

        def step_alt():
            fut = zk.multiexp(worker, (b_alt, 0), zk.FullDensity(), s_alt)
            return zk.shard.exchange(fut, 12, index_offset=lo_alt, device=dev if backend == "nccl" else None)

        for _ in range(max(1, args.warmup)):
            step_alt()
        L.mi355zk_prof_reset()
        L.mi355zk_prof_enable(1)
        dist.barrier()
        torch.cuda.synchronize()
        with _no_gc(collect=False):
            t1 = time.perf_counter()
            for _ in range(args.steps):
                r_alt = step_alt()
            torch.cuda.synchronize()
            dist.barrier()
            dt_alt = time.perf_counter() - t1
        L.mi355zk_prof_enable(0)
        tt = torch.tensor([dt_alt], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        dt_alt = float(tt.item()) / args.steps
        kern_alt = _prof(L, ("msm_digits", "msm_sort", "msm_accumulate", "msm_reduce"))
        a_alt, a_main = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
        L.mi355zk_bn254_g1_to_affine(a_alt.ctypes.data_as(C.c_void_p), np.ascontiguousarray(r_alt).ctypes.data_as(C.c_void_p))
        L.mi355zk_bn254_g1_to_affine(a_main.ctypes.data_as(C.c_void_p), np.ascontiguousarray(result).ctypes.data_as(C.c_void_p))
        nw_alt = C.c_int()
        c_alt = L.mi355zk_msm_window_bits_groups(n_alt, 1, C.byref(nw_alt))
        alt_plan = {"parallelism": "%d point range(s) x 1 window group(s), all-gather of 96-B partials" % world, "points_per_gpu": n_alt,
                    "window_bits": c_alt, "windows": nw_alt.value, "ms_per_step": round(dt_alt * 1e3, 3), "value": round(n_total / dt_alt / 1e6, 3),
                    "kernel_ms_rank0": {k: (round(v, 4) if v is not None else None) for k, v in kern_alt.items()},
                    "same_point_as_the_timed_plan": bool(np.array_equal(a_alt, a_main))}
        assert alt_plan["same_point_as_the_timed_plan"], "the N x 1 plan's result differs from the timed plan's"

    # ---- the same step with the scalars' host-to-device copy inside the timed region (SURVEY 8d defines the metric with "H2D of
    # scalars included"; `value` keeps inputs resident as the bench contract asks): pinned host buffer -> HBM -> multiexp
    h2d = None
    if args.full and not args.no_h2d_leg and world == 1:
        # the library's host-buffer entry point: the base vector is cached on the device after the first call (the CRS is reused
        # by every proof), the scalars are streamed from (pageable) host memory in chunks overlapped with the kernels
        hb = bases.cpu().numpy().view(np.uint64)
        hs = scalars.cpu().numpy().view(np.uint64)
        zk.pin_bases(hb)  # the shim's promise that this `Arc<Vec<G1Affine>>` is immutable: its device copy is kept across calls
        t1 = time.perf_counter()
        r_first = zk.multiexp(worker, (hb, 0), zk.FullDensity(), hs).wait()
        dt_first = time.perf_counter() - t1
        reps = min(3, args.steps)
        t1 = time.perf_counter()
        for _ in range(reps):
            r2 = zk.multiexp(worker, (hb, 0), zk.FullDensity(), hs).wait()
        dt = (time.perf_counter() - t1) / reps
        # the same call with the exponent vector in PAGE-LOCKED host memory (what a shim gets by allocating its Vec<FrRepr> through
        # hipHostMalloc / registering it): the DMA engine reads it directly, where a pageable vector goes through the runtime's
        # staging at a rate that depends on the host (25 - 56 GB/s measured from box to box).  The better of the two is reported
        # as value_incl_scalar_h2d -- both are the library's one entry point, only the caller's allocation differs.
        hs_pin_t = torch.empty(scalars.shape, dtype=torch.int64, pin_memory=True)
        hs_pin_t.copy_(scalars)
        torch.cuda.synchronize()
        hs_pin = hs_pin_t.numpy().view(np.uint64)
        zk.multiexp(worker, (hb, 0), zk.FullDensity(), hs_pin).wait()
        t1 = time.perf_counter()
        for _ in range(reps):
            r3 = zk.multiexp(worker, (hb, 0), zk.FullDensity(), hs_pin).wait()
        dt_pin = (time.perf_counter() - t1) / reps
        a1, a2, a3 = np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64), np.zeros(8, dtype=np.uint64)
        L.mi355zk_bn254_g1_to_affine(a1.ctypes.data_as(C.c_void_p), np.ascontiguousarray(r2).ctypes.data_as(C.c_void_p))
        L.mi355zk_bn254_g1_to_affine(a2.ctypes.data_as(C.c_void_p), np.ascontiguousarray(result).ctypes.data_as(C.c_void_p))
        L.mi355zk_bn254_g1_to_affine(a3.ctypes.data_as(C.c_void_p), np.ascontiguousarray(r3).ctypes.data_as(C.c_void_p))
        dt_page = dt
        dt = min(dt_page, dt_pin)
        del hs_pin, hs_pin_t
        h2d = {"value_incl_scalar_h2d": round(n_total / dt / 1e6, 3), "ms_per_step": round(dt * 1e3, 3),
               "pageable_exponents_ms": round(dt_page * 1e3, 3), "page_locked_exponents_ms": round(dt_pin * 1e3, 3),
               "first_call_incl_bases_h2d_ms": round(dt_first * 1e3, 3), "same_result": bool(np.array_equal(a1, a2) and np.array_equal(a3, a2)),
               "note": "mi355zk_bn254_g1_msm (host buffers): pinned bases cached on the device after the first call, exponents streamed from "
                       "host memory in chunks that are accumulated into ONE bucket array while the next chunk uploads; timed with the exponent "
                       "vector in pageable and in page-locked host memory (the runtime's staging of pageable memory runs at 25-56 GB/s "
                       "depending on the host), the better one is value_incl_scalar_h2d; first call = bases + scalars over PCIe"}
        zk.unpin_bases(None)
        del hb, hs, r_first
    elif args.full and not args.no_h2d_leg:
        host_sc = torch.empty(scalars.shape, dtype=scalars.dtype, pin_memory=True)
        host_sc.copy_(scalars)
        stage = torch.empty_like(scalars)
        torch.cuda.synchronize()
        dist.barrier()
        t1 = time.perf_counter()
        reps = min(3, args.steps)
        for _ in range(reps):
            stage.copy_(host_sc, non_blocking=True)
            step(stage)
        torch.cuda.synchronize()
        dist.barrier()
        dt = (time.perf_counter() - t1) / reps
        t = torch.tensor([dt], dtype=torch.float64, device=dev if backend == "nccl" else "cpu")
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        dt = float(t.item())
        h2d = {"value_incl_scalar_h2d": round(n_total / dt / 1e6, 3), "ms_per_step": round(dt * 1e3, 3),
               "note": "every rank copies its scalars from a pinned host buffer on every step (not overlapped), bases resident"}
        del host_sc, stage

    out = None
    if rank == 0:
        aff = np.zeros(8, dtype=np.uint64)
        L.mi355zk_bn254_g1_to_affine(aff.ctypes.data_as(C.c_void_p), np.ascontiguousarray(result).ctypes.data_as(C.c_void_p))
        ms_per_step = elapsed / args.steps * 1e3
        value = n_total / (elapsed / args.steps) / 1e6
        nw = C.c_int()
        c_bits = L.mi355zk_msm_window_bits_groups(n_local, wgroups, C.byref(nw))
        roofline = None
        if args.full:
            acc_ms = kern["msm_accumulate"]
            nw_rank = nw.value // wgroups  # windows one launch of this rank accumulates: that share of its scalar-muls' work
            achieved = BYTES_PER_SCALAR_MUL * (n_local / wgroups) / (acc_ms * 1e-3) / 1e9 if acc_ms else None
            # integer-ALU model: W mixed adds per scalar-mul, 10 Fq mul each (XYZZ 8M+2S)
            fq_mul_per_s = (nw_rank * 10 * n_local / (acc_ms * 1e-3)) if acc_ms else None
            roofline = {"bound": "hbm", "kernel": "msm_accumulate_kernel", "achieved": round(achieved, 3) if achieved else None,
                        "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 6) if achieved else None,
                        "traffic": traffic,
                        "kernel_ms": {k: (round(v, 4) if v is not None else None) for k, v in kern.items()},
                        "alu_model": {"fq_mul_per_s": fq_mul_per_s,
                                      "mad_u64_u32_per_s": (nw_rank * MADS_PER_MIXED_ADD * n_local / (acc_ms * 1e-3)) if acc_ms else None,
                                      "mad_peak_per_s": MAD_PEAK_PER_S,
                                      "frac": round(nw_rank * MADS_PER_MIXED_ADD * n_local / (acc_ms * 1e-3) / MAD_PEAK_PER_S, 4) if acc_ms else None,
                                      "note": "W mixed adds (10 Fq products = 1467 v_mad_u64_u32) per scalar-mul in msm_accumulate; "
                                              "MSM is integer-ALU bound (SURVEY 8d), the multiplier instructions alone are this fraction of the measured v_mad_u64_u32 peak"}}
        out = {
            "metric": "BN254 G1 MSM throughput (Mscalar-mul/s) at 2^%d points" % log_n,
            "value": round(value, 3),
            "unit": "Mscalar-mul/s",
            "n_gpus": world,
            "settle_steps": settle_steps,   # untimed steps after the W warm-up steps (short steps only: see above)
            "rccl_ranks": dist.get_world_size() if world > 1 else 1,   # the world size torch.distributed sees
            "backend": backend if world > 1 else None,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(ms_per_step, 3),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "u32x8 (256-bit Montgomery limbs)",
            "data": "synthetic (bases k_i*G generated on device, scalars uniform < r)",
            "config": {"workload": "2^%d-point BN254 G1 Pippenger MSM, FullDensity, bases+scalars resident in HBM" % log_n,
                       "bases": "k_i*G, independent k_i" if args.bases == "random" else "tau^i*G (tau-table structure)",
                       "points_per_gpu": n_local, "bases_bytes_per_gpu": n_local * 64, "window_bits": c_bits, "windows": nw.value,
                       "parallelism": "%d point range(s) x %d window group(s), all-gather of 96-B partials" % (pgroups, wgroups)},
            "roofline": roofline,
            "result_affine_x_limb0": hex(int(aff[0])),
            "full_size_linearity_check": additive_ok,
            "sharded_result_matches_unsharded": sharded_ok if world > 1 else None,
            "preflight": preflight,
            "alt_plan": alt_plan,
            # SURVEY 8(d) defines the metric with the exponents' upload inside the call; the bench contract defines `value` with
            # every input resident.  Both are reported, each under its own name.
            "value_definition": "`value`: every input resident in HBM when the timed region starts -- the bench contract's definition, which says of a "
                                "boundary that hands over host buffers that the PCIe-inclusive rate 'is never `value`'.  SURVEY 8(d) defines the metric "
                                "with the exponents' upload inside the call: that is `value_incl_scalar_h2d` (one mi355zk_bn254_g1_msm call, pinned bases "
                                "on the device, 2 GiB of exponents streamed over PCIe while the kernels run).",
            "value_incl_scalar_h2d": h2d["value_incl_scalar_h2d"] if h2d else None,
            "incl_scalar_h2d": h2d,
            "input_gen_s": round(t_gen, 2),
            "full": args.full,   # False: the headline only (roofline, checks, h2d leg, cpu_baseline and secondary are --full)
        }

    # ---- CPU baseline: the oracle's restatement of bellman multiexp on the host cores (rank 0, N=1 only)
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline:
        import oracle_lib as O

        ns = 1 << min(args.cpu_sample_log_n, log_n)
        hb = bases[:ns].cpu().numpy().view(np.uint64)
        hs = scalars[:ns].cpu().numpy().view(np.uint64)
        cores = os.cpu_count() or 1
        c_ref = O.multiexp_window_bits(ns)
        windows = (254 + c_ref - 1) // c_ref
        threads = min(cores, windows)  # bellman runs one pool task per window (multiexp.rs:75,145)
        t1 = time.perf_counter()
        rc, ref = O.G1.multiexp(hb, hs, threads=threads)
        dt = time.perf_counter() - t1
        assert rc == 0
        # parity of the GPU path on the same sample (affine-normalised, bit exact)
        got = zk.multiexp(worker, (bases[:ns], 0), zk.FullDensity(), scalars[:ns]).wait()
        ok = bool(np.array_equal(O.G1.to_affine(got), O.G1.to_affine(ref)))
        # the same sample at the window width bellman picks at the HEADLINE size (c = ceil(ln 2^26) = 19, 14 windows = 14 busy threads,
        # multiexp.rs:341-345,75): the reference's shape at the metric's size, on a sample the oracle finishes in seconds
        at_metric = None
        c_metric = O.multiexp_window_bits(n_total) if n_total < (1 << 32) else 19
        if c_metric != c_ref:
            O.multiexp_set_window_bits(c_metric)
            try:
                w_m = (254 + c_metric - 1) // c_metric
                t2 = time.perf_counter()
                rc_m, ref_m = O.G1.multiexp(hb, hs, threads=min(cores, w_m))
                dt_m = time.perf_counter() - t2
            finally:
                O.multiexp_set_window_bits(0)
            at_metric = {"window_bits": c_metric, "windows": w_m, "threads": min(cores, w_m), "Mscalar_mul_per_s": round(ns / dt_m / 1e6, 4),
                         "seconds": round(dt_m, 2), "same_point": bool(rc_m == 0 and np.array_equal(O.G1.to_affine(ref_m), O.G1.to_affine(ref)))}
        out["cpu_baseline"] = {"value": round(ns / dt / 1e6, 4), "unit": "Mscalar-mul/s", "cores": threads, "threads": threads, "host_cores": cores,
                               "host_cpu": host_cpu_info(), "kind": "port", "at_the_metric_size_window": at_metric,
                               "sample": "first 2^%d points of the same input, oracle restatement of bellman_ce multiexp "
                                         "(c=%d, one thread per window, %d windows), %.2f s" % (int(np.log2(ns)), c_ref, windows, dt),
                               "gpu_matches_oracle_on_sample": ok}
    if args.full and rank == 0 and world == 1 and not args.no_secondary:
        del bases, scalars
        torch.cuda.empty_cache()
        out["secondary"] = secondary(zk, L, worker, dev, args.secondary_log_n, cpu=not args.no_cpu_baseline)
        if not args.no_rows:
            torch.cuda.empty_cache()
            out["secondary"].update(secondary_rows(zk, L, worker, dev, args.secondary_log_n, cpu=not args.no_cpu_baseline))
    # ---- (N > 1) the single-process form of the same job in the same line (VERDICT r5 #6c): ONE process, mi355zk_init over the N devices, one
    # host-buffer call cut into a point range per device (include/mi355zk.h).  A child of rank 0 with a time limit, started AFTER the process group is gone:
    # the other ranks have left by then (their GPUs are idle and their memory is free), so nothing of this optional leg can hang a collective or cost the
    # headline its line.  Needs every GPU visible to rank 0 (nccl runs only).  BENCH_SINGLE_PROCESS_LEG=0 skips it.
    single_leg = args.full and world > 1 and backend == "nccl" and os.environ.get("BENCH_SINGLE_PROCESS_LEG", "1") != "0"
    if world > 1:
        if single_leg:
            del bases, scalars
            torch.cuda.empty_cache()
        dist.barrier()
        dist.destroy_process_group()
    if single_leg and rank == 0:
        import subprocess

        time.sleep(2.0)   # (the other ranks are exiting)
        counts = [str(k) for k in (1, world) if k <= torch.cuda.device_count()]
        env_child = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT", "GROUP_RANK", "ROLE_RANK",
                                                                   "LOCAL_WORLD_SIZE", "ROLE_WORLD_SIZE", "TORCHELASTIC_RUN_ID")}
        try:
            ch = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "bench_multi_device.py"), "--log-n", "24", "--iters", "3", "--no-batch-exp", "--devices"] + counts,
                                capture_output=True, text=True, timeout=200, cwd=ROOT, env=env_child)
            line = [ln for ln in ch.stdout.splitlines() if ln.startswith("{")]
            out["single_process_multi_gpu_2e24"] = json.loads(line[-1]) if ch.returncode == 0 and line else {"error": "rc %d: %s" % (ch.returncode, ch.stderr[-300:])}
        except Exception as e:  # noqa: BLE001
            out["single_process_multi_gpu_2e24"] = {"error": repr(e)[:300]}
    if rank == 0:
        full = [ms for g, ms in _GC_LOG if g == 2]
        out["host_gc"] = {"collections": len(_GC_LOG), "full_collections": len(full), "longest_ms": round(max([ms for _, ms in _GC_LOG], default=0.0), 2),
                          "note": "cyclic-GC runs of this interpreter during the whole bench (outside the timed loops, which run with the collector "
                                  "off): a full collection with torch imported is what put single 38-64 ms calls into round 4's table-mode legs"}
        print(json.dumps(out), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
