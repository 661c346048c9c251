#!/usr/bin/env python3
"""The prover's H-polynomial chain (prover.rs:216-248) on one MI355X: the single-call entry points against what they replace.

Rows (per size; median, min and max over --rounds samples, the rows of a group alternating inside every round so that they see the same clocks
and the same neighbours on the host):
  a  composed_dev    the device chain as ten entry-point calls: ifft and coset_fft batched over a, b, c, mul_assign, sub_assign,
                     divide_by_z_on_coset, icoset_fft
  b  h_poly_dev      mi355zk_bn254_fr_h_poly_dev
  c  elementwise3    mul_assign + sub_assign + divide_by_z_on_coset alone      c1  h_combine  mi355zk_bn254_fr_h_combine_dev alone
  d  domain_op_x7    seven mi355zk_bn254_fr_domain_op calls on pageable host arrays (the drop-in path WITHOUT its CPU elementwise work: a floor for it)
  e  h_poly_host     mi355zk_bn254_fr_h_poly from pageable host arrays (into_repr)
  f  pinned_copy     96 * n bytes up and 32 * n bytes down between pinned host memory and the device: the link floor of e
A library without the new symbols (MI355ZK_SO=<the parent's build>) runs rows a, c, d, f and reports the others as null.
Device rows time --inner back-to-back chains between two synchronisations (no per-call events); host rows are synchronous calls."""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import phase2_bn254_amd as zk, inputs

ap = argparse.ArgumentParser()
ap.add_argument("--log-n", type=int, nargs="+", default=[16, 20]); ap.add_argument("--rounds", type=int, default=15); ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--warm-ms", type=float, default=50.0); ap.add_argument("--out", default=None)
A = ap.parse_args()
so = C.CDLL(zk.lib.SO_PATH)   # (raw handle: lib.load() binds every declared symbol and would refuse the parent's library)
HAVE_NEW = hasattr(so, "mi355zk_bn254_fr_h_poly")
if HAVE_NEW:
    L = zk.lib.load()
else:
    L = so
    for name, (res, args) in zk.lib.SIGNATURES.items():
        if hasattr(so, name):
            getattr(so, name).restype, getattr(so, name).argtypes = res, args
    assert L.mi355zk_init(None, 0) == 0
vp = C.c_void_p


def stats(samples):
    s = sorted(samples)
    return {"median_ms": round(statistics.median(s) * 1e3, 4), "min_ms": round(s[0] * 1e3, 4), "max_ms": round(s[-1] * 1e3, 4), "samples": len(s)}


def run_size(log_n):
    n = 1 << log_n
    host = [inputs.random_fr_mont(n, seed=70 + k) for k in range(3)]
    d = [torch.from_numpy(x.view(np.int64)).cuda() for x in host]
    p = [vp(t.data_ptr()) for t in d]
    ptrs = (vp * 3)(*[t.data_ptr() for t in d])

    def chk(rc):
        assert rc == 0, rc

    def elementwise3():
        chk(L.mi355zk_bn254_fr_mul_assign_dev(p[0], p[1], n, None)); chk(L.mi355zk_bn254_fr_sub_assign_dev(p[0], p[2], n, None))
        chk(L.mi355zk_bn254_fr_divide_by_z_on_coset_dev(p[0], log_n, None))

    def composed_dev():
        chk(L.mi355zk_bn254_fr_domain_op_batch_dev(ptrs, 3, log_n, zk.lib.OP_IFFT, None)); chk(L.mi355zk_bn254_fr_domain_op_batch_dev(ptrs, 3, log_n, zk.lib.OP_COSET_FFT, None))
        elementwise3()
        chk(L.mi355zk_bn254_fr_domain_op_dev(p[0], log_n, zk.lib.OP_ICOSET_FFT, None))

    def h_poly_dev():
        chk(L.mi355zk_bn254_fr_h_poly_dev(p[0], p[1], p[2], log_n, 0, None))

    def h_combine():
        chk(L.mi355zk_bn254_fr_h_combine_dev(p[0], p[1], p[2], n, log_n, None))

    work = [x.copy() for x in host]   # pageable; row d transforms them in place (any Fr values do), row e only reads them
    hp = [x.ctypes.data_as(vp) for x in work]
    h_out = np.empty((n, 4), dtype=np.uint64)

    def domain_op_x7():
        for k in range(3):
            chk(L.mi355zk_bn254_fr_domain_op(hp[k], log_n, zk.lib.OP_IFFT)); chk(L.mi355zk_bn254_fr_domain_op(hp[k], log_n, zk.lib.OP_COSET_FFT))
        chk(L.mi355zk_bn254_fr_domain_op(hp[0], log_n, zk.lib.OP_ICOSET_FFT))

    def h_poly_host():
        chk(L.mi355zk_bn254_fr_h_poly(h_out.ctypes.data_as(vp), hp[0], hp[1], hp[2], n, log_n, zk.lib.H_INTO_REPR))

    pin_up = torch.empty((3 * n, 4), dtype=torch.int64).pin_memory(); pin_up.copy_(torch.from_numpy(np.concatenate(host).view(np.int64)))
    pin_dn = torch.empty((n, 4), dtype=torch.int64).pin_memory()
    d_up = torch.empty((3 * n, 4), dtype=torch.int64, device="cuda")

    def pinned_copy():
        d_up.copy_(pin_up, non_blocking=True); pin_dn.copy_(d_up[:n], non_blocking=True); torch.cuda.synchronize()

    dev_rows = [("a_composed_dev", composed_dev, True), ("b_h_poly_dev", h_poly_dev, HAVE_NEW), ("c_elementwise3", elementwise3, True), ("c1_h_combine", h_combine, HAVE_NEW)]
    host_rows = [("d_domain_op_x7", domain_op_x7, True), ("e_h_poly_host", h_poly_host, HAVE_NEW), ("f_pinned_copy", pinned_copy, True)]
    res = {name: None for name, _, _ in dev_rows + host_rows}
    dev_rows = [r for r in dev_rows if r[2]]; host_rows = [r for r in host_rows if r[2]]
    # warm-up: every row once (tables, code objects, pools), then --warm-ms of device work so that the clocks are up (tools/bench_ntt.py)
    for _, fn, _ in dev_rows + host_rows: fn()
    t_warm = time.perf_counter() + A.warm_ms * 1e-3
    while time.perf_counter() < t_warm: composed_dev()
    torch.cuda.synchronize()
    samples = {name: [] for name, _, _ in dev_rows + host_rows}
    for _ in range(A.rounds):
        for name, fn, _ in dev_rows:
            fn(); torch.cuda.synchronize()
            t = time.perf_counter()
            for _ in range(A.inner): fn()
            torch.cuda.synchronize(); samples[name].append((time.perf_counter() - t) / A.inner)
        for name, fn, _ in host_rows:
            t = time.perf_counter(); fn(); samples[name].append(time.perf_counter() - t)
    for name, s in samples.items(): res[name] = stats(s)
    med = lambda k: res[k]["median_ms"] if res[k] else None   # noqa: E731
    ratios = {"bytes_up_down_MiB": {"d": round(7 * 2 * 32 * n / 2**20, 1), "e": round(4 * 32 * n / 2**20, 1)}}
    if HAVE_NEW:
        ratios.update({"b_over_a": round(med("b_h_poly_dev") / med("a_composed_dev"), 4), "c_over_c1": round(med("c_elementwise3") / med("c1_h_combine"), 3),
                       "d_over_e": round(med("d_domain_op_x7") / med("e_h_poly_host"), 3), "e_over_f": round(med("e_h_poly_host") / med("f_pinned_copy"), 3),
                       "h_combine_GBs": round(128 * n / (med("c1_h_combine") * 1e-3) / 1e9, 1)})
    ratios["elementwise3_GBs"] = round(256 * n / (med("c_elementwise3") * 1e-3) / 1e9, 1)
    return {"log_n": log_n, "rows": res, "derived": ratios}


out = {"device": torch.cuda.get_device_name(0), "library": os.path.relpath(zk.lib.SO_PATH, ROOT), "has_h_poly": HAVE_NEW, "rounds": A.rounds, "inner": A.inner,
       "warm_ms": A.warm_ms, "sizes": [run_size(k) for k in A.log_n]}
line = json.dumps(out)
print(line)
if A.out:
    with open(A.out, "w") as f: f.write(json.dumps(out, indent=1) + "\n")
