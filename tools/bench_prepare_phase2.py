#!/usr/bin/env python3
"""prepare_phase2 streamed file to files on one MI355X against the in-memory flow -> profiles/prepare_phase2.md.

  1  stream.prepare_phase2_files at --power (20), every degree, from a compressed response: wall time, split into load (points_load),
     transforms (point_ifft), H bases (shifted_difference) and store (points_store); what is left is the device copies, the file creation
     and Python.  Beside it the sum of ceremony.prepare_phase2 over the same degrees on an accumulator already decoded in HBM (reading the
     file and writing the results are not charged to it).
  2  the H bases alone at shift = 2^power: ceremony.shifted_difference against the two-term rows of ceremony.eval_qap (building the index
     and coefficient arrays charged separately), with the bytes each route takes from the device.
  3  the low-water mark of torch.cuda.mem_get_info() over the first streamed run at --power of this process (sampled every 2 ms from a
     thread), next to Phase2Plan.device_bytes().  The input files are made by child processes and the only work before it is one streamed
     run of a power-4 file, which loads the code objects and creates the streams: no pool of this process has grown past that before.

Times are medians of --iters runs after --warm runs, in ms, from a host clock around work that ends in a device synchronise; no figure is a
gate.  Power 28 is not run."""
import argparse, json, os, statistics, subprocess, sys, tempfile, threading, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
ap = argparse.ArgumentParser()
ap.add_argument("--power", type=int, default=20); ap.add_argument("--piece", type=int, default=0)
ap.add_argument("--iters", type=int, default=2); ap.add_argument("--warm", type=int, default=1); ap.add_argument("--dir", default=None)
ap.add_argument("--make", default=None, help="(internal) write the response file here and exit")
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prepare_phase2.md"))
a = ap.parse_args()

import numpy as np, torch  # noqa: E402
import phase2_bn254_amd as zk  # noqa: E402
zk.lib.load(); zk.Worker(0)
SECRETS = (0xABCDEF123456789, 0x1111222233334444, 0x9999AAAABBBB)

if a.make:
    zk.new_constrained(a.make + ".challenge", a.power, 1 << 18)
    zk.compute_constrained(a.make + ".challenge", a.make, a.power, 1 << 18, *SECRETS)
    os.remove(a.make + ".challenge")
    sys.exit(0)

PARTS = ("load", "transforms", "h bases", "store")
spent = dict.fromkeys(PARTS, 0.0)


def charged(name, fn):
    def wrapper(*args, **kwargs):
        torch.cuda.synchronize(); t = time.perf_counter()
        try:
            return fn(*args, **kwargs)
        finally:
            torch.cuda.synchronize(); spent[name] += (time.perf_counter() - t) * 1e3
    return wrapper


class LowWater:
    """the least free device memory seen while the block runs, sampled from a thread"""
    def __enter__(self):
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        self.start = self.low = torch.cuda.mem_get_info()[0]
        self.stop = False
        dev = torch.cuda.current_device()

        def poll():
            torch.cuda.set_device(dev)
            while not self.stop:
                self.low = min(self.low, torch.cuda.mem_get_info()[0]); time.sleep(0.002)
        self.thread = threading.Thread(target=poll); self.thread.start()
        return self

    def __exit__(self, *exc):
        self.stop = True; self.thread.join()
        torch.cuda.synchronize(); self.low = min(self.low, torch.cuda.mem_get_info()[0])   # (a call shorter than the sampling period: what it returned is still held here)
        self.used = self.start - self.low
        torch.cuda.synchronize(); torch.cuda.empty_cache()
        self.kept = self.start - torch.cuda.mem_get_info()[0]   # what the process still holds afterwards (pools, the runtime's own)


def note(*what):
    print(*what, file=sys.stderr, flush=True)


def run_timed(fn, iters, warm):
    rows = []
    for _ in range(warm + iters):
        for k in spent: spent[k] = 0.0
        torch.cuda.synchronize(); t = time.perf_counter(); fn(); torch.cuda.synchronize()
        rows.append({"total": (time.perf_counter() - t) * 1e3, **spent})
        note("run", rows[-1])
    rows = rows[warm:]
    return {k: round(statistics.median(r[k] for r in rows), 1) for k in rows[0]}


with tempfile.TemporaryDirectory(dir=a.dir) as d:
    response = os.path.join(d, "response")
    subprocess.run([sys.executable, os.path.abspath(__file__), "--power", str(a.power), "--make", response], check=True)
    subprocess.run([sys.executable, os.path.abspath(__file__), "--power", "4", "--make", response + "4"], check=True)
    zk.prepare_phase2_files(response + "4", os.path.join(d, "warm"), 4, piece=a.piece)
    plan = zk.prepare_phase2_plan(a.power)
    runs = [0]

    def streamed():
        runs[0] += 1
        out = os.path.join(d, "out%d" % runs[0])
        zk.prepare_phase2_files(response, out, a.power, piece=a.piece)
        for name in os.listdir(out): os.remove(os.path.join(out, name))

    # ---- 3 first: nothing of this process has touched the pools yet
    with LowWater() as water:
        streamed()
    note("first streamed run: low water", water.used, "kept", water.kept)
    # ---- 1
    real = (zk.stream.points_load, zk.ceremony.point_ifft, zk.ceremony.shifted_difference, zk.stream.points_store)
    zk.stream.points_load = charged("load", real[0]); zk.ceremony.point_ifft = charged("transforms", real[1])
    zk.ceremony.shifted_difference = charged("h bases", real[2]); zk.stream.points_store = charged("store", real[3])
    m1 = run_timed(streamed, a.iters, a.warm)
    zk.stream.points_load, zk.ceremony.point_ifft, zk.ceremony.shifted_difference, zk.stream.points_store = real
    torch.cuda.empty_cache()
    acc = zk.ceremony.read_accumulator(zk.verify._file_tensor(open(response, "rb").read()), a.power, compressed=True)
    zk.ceremony.point_ifft = charged("transforms", real[1])

    def in_memory():
        for k in range(a.power + 1):
            zk.ceremony.prepare_phase2(acc, 1 << k)

    m1_mem = run_timed(in_memory, a.iters, a.warm)
    zk.ceremony.point_ifft = real[1]
    # ---- 2: the H bases of the largest degree, both routes over the same vector
    m = 1 << a.power
    n_h = m - 1
    tau_g1 = acc["tau_g1"].contiguous()
    dev = tau_g1.device

    def indices():
        r_minus_1 = [0x43E1F593F0000000, 0x2833E84879B97091, 0xB85045B68181585D, 0x30644E72E131A029]
        to_i64 = lambda limbs: [v - (1 << 64) if v >= (1 << 63) else v for v in limbs]  # noqa: E731
        coeff = torch.tensor([to_i64([1, 0, 0, 0]), to_i64(r_minus_1)], dtype=torch.int64, device=dev).repeat(n_h, 1).contiguous()
        idx = torch.arange(n_h, device=dev, dtype=torch.int32)
        return (2 * torch.arange(n_h + 1, device=dev, dtype=torch.int32)).contiguous(), torch.stack([idx + m, idx], dim=1).reshape(-1).contiguous(), coeff

    def time_of(fn):
        ts = []
        for _ in range(a.warm + a.iters + 2):
            torch.cuda.synchronize(); t = time.perf_counter(); r = fn(); torch.cuda.synchronize(); ts.append((time.perf_counter() - t) * 1e3)
        return round(statistics.median(ts[a.warm:]), 2), r

    note("in memory done")
    t_idx, (row_ptr, col, coeff) = time_of(indices)
    index_bytes = sum(t.numel() * t.element_size() for t in (row_ptr, col, coeff))
    t_sparse, want = time_of(lambda: zk.ceremony.eval_qap(tau_g1, row_ptr, col, coeff))
    with LowWater() as water_sparse:
        held = zk.ceremony.eval_qap(tau_g1, row_ptr, col, coeff)
    del row_ptr, col, coeff
    t_diff, got = time_of(lambda: zk.ceremony.shifted_difference(tau_g1, m, n_h))
    with LowWater() as water_diff:
        held = zk.ceremony.shifted_difference(tau_g1, m, n_h)
    del held
    same = bool(torch.equal(got, want))

rocm = open("/opt/rocm/.info/version").read().strip() if os.path.exists("/opt/rocm/.info/version") else "unknown"
MiB = 2.0 ** 20
with open(a.out, "w") as f:
    f.write("# prepare_phase2, file to files: measurements\n\nWritten by `tools/bench_prepare_phase2.py --power %d --piece %d` on %s (ROCm %s, torch %s): medians of %d runs after "
            "%d warm-up runs, ms, host clock around work that ends in a device synchronise.  Response %.0f MiB in, %d files, %.0f MiB out.\n\n"
            % (a.power, a.piece, torch.cuda.get_device_name(0), rocm, torch.__version__, a.iters, a.warm, plan.input_size / MiB, len(plan.files),
               sum(x.size for x in plan.files.values()) / MiB))
    f.write("## 1. Every degree 0 .. %d\n\n| flow | total | load | transforms | h bases | store | rest |\n|---|---|---|---|---|---|---|\n" % a.power)
    rest = round(m1["total"] - sum(m1[k] for k in PARTS), 1)
    f.write("| prepare_phase2_files (compressed response file -> radix files) | %s | %s | %s | %s | %s | %s |\n" % (m1["total"], m1["load"], m1["transforms"], m1["h bases"], m1["store"], rest))
    f.write("| sum of ceremony.prepare_phase2 (accumulator decoded in HBM, results left in HBM) | %s | - | %s | (sparse product, inside the rest) | - | %s |\n\n"
            % (m1_mem["total"], m1_mem["transforms"], round(m1_mem["total"] - m1_mem["transforms"], 1)))
    f.write("## 2. The H bases of degree 2^%d (%d outputs)\n\n| route | ms | device bytes beyond the input vector and the output |\n|---|---|---|\n" % (a.power, n_h))
    f.write("| shifted_difference kernel | %s | %.1f MiB measured (low water, output of %.1f MiB subtracted; the unit allocates nothing) |\n" % (t_diff, max(0, water_diff.used - 64 * n_h) / MiB, 64 * n_h / MiB))
    f.write("| eval_qap over two-term rows | %s (+ %s to build the arrays) | %.1f MiB of row pointers, columns and coefficients + %.1f MiB measured during the product (low water, output subtracted) |\n\n"
            % (t_sparse, t_idx, index_bytes / MiB, max(0, water_sparse.used - 64 * n_h) / MiB))
    f.write("Both routes give the same bytes: %s.\n\n" % same)
    f.write("## 3. Device memory of the first streamed run\n\nLow-water mark of `torch.cuda.mem_get_info()` (2 ms samples): %.1f MiB below the start; %.1f MiB are still held after the run "
            "(the pooled piece buffer and what the runtime keeps).  `Phase2Plan.device_bytes(%d)`: %.1f MiB.\n"
            % (water.used / MiB, water.kept / MiB, a.piece, plan.device_bytes(a.piece) / MiB))
result = {"power": a.power, "streamed": m1, "in_memory": m1_mem, "h_kernel_ms": t_diff, "h_sparse_ms": t_sparse, "h_index_build_ms": t_idx, "h_index_bytes": index_bytes,
          "h_same_bytes": same, "h_kernel_extra_bytes": water_diff.used - 64 * n_h, "h_sparse_extra_bytes": water_sparse.used - 64 * n_h,
          "low_water_bytes": water.used, "kept_bytes": water.kept, "plan_device_bytes": plan.device_bytes(a.piece)}
print(json.dumps(result), flush=True)
