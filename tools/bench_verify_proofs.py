#!/usr/bin/env python3
"""Groth16 verification of n proofs against one key on one MI355X: pairing.verify_proofs (the baseline: host input accumulators, one
pairing launch), verify_proofs_dev (accumulators on the device) and verify_proofs_batch (n + 3 Miller loops, one final exponentiation), for
n = 2^k (--sizes) and l public inputs (--inputs); then the accumulator launch alone (mi355zk_bn254_g1_fixed_bases_lincomb_dev) against
FixedBaseTable.mul once per input (l launches and NO additions: a lower bound of what the single-base tables can do), and the slice plan
A/B: one combination shape under forced slice lengths beside the planned one.  Timing as tools/bench_pairing.py: median and minimum of
--iters calls to a synchronised stream after --warm calls and --warm-ms more.  The baseline costs seconds per call: it runs ONCE, and above
--baseline-max proofs on a PREFIX of that many, scaled to n (the row says so).  Proofs are simulated over a key with known logarithms
(tests/test_gpu_verify_proofs.py); every path's verdicts are checked.  One JSON line per row."""
import argparse, ctypes as C, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import phase2_bn254_amd as zk, inputs

ap = argparse.ArgumentParser()
ap.add_argument("--sizes", default="10,14,16"); ap.add_argument("--inputs", default="1,16"); ap.add_argument("--iters", type=int, default=5)
ap.add_argument("--warm", type=int, default=2); ap.add_argument("--warm-ms", type=float, default=200.0); ap.add_argument("--baseline-max", type=int, default=1024)
ap.add_argument("--plan-shapes", default="1x1000,1x64,64x1000,1024x16,16384x16,65536x16,262144x4"); ap.add_argument("--plan-slices", default="0,1,2,4,8,16,32,64,all")
a = ap.parse_args()
L = zk.lib.load(); w = zk.Worker(0)
R = zk.prover._R_ORDER
ALPHA, BETA, GAMMA, DELTA = 0x1B7E4D3C2A190807F6E5D4C3B2A1908F % R, 0x2468ACE013579BDF02468ACE13579BDF % R, 0x0123456789ABCDEF0FEDCBA987654321 % R, R - 0x5DEECE66D
KEY = bytes(range(32))


def ints(rows):
    return [sum(int(v) << (64 * i) for i, v in enumerate(row)) for row in np.asarray(rows, dtype=np.uint64).reshape(-1, 4)]


def limbs(vals):
    return np.array([[(int(v) % R >> (64 * i)) & ((1 << 64) - 1) for i in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def mul(group, scalars):
    gen = np.ascontiguousarray(inputs.G1_GEN_RAW if group == 1 else inputs.G2_GEN_RAW)
    fn = L.mi355zk_bn254_g1_batch_mul_dev if group == 1 else L.mi355zk_bn254_g2_batch_mul_dev
    k = torch.from_numpy(limbs(scalars).view(np.int64)).cuda()
    p = torch.empty((k.shape[0], 8 * group), dtype=torch.int64, device="cuda")
    assert fn(C.c_void_p(p.data_ptr()), gen.ctypes.data_as(C.c_void_p), C.c_void_p(k.data_ptr()), k.shape[0], None) == 0
    torch.cuda.synchronize()
    return p


def timed(fn):
    for _ in range(a.warm): fn()
    torch.cuda.synchronize()
    t_warm = time.perf_counter() + a.warm_ms * 1e-3
    while time.perf_counter() < t_warm: fn(); torch.cuda.synchronize()
    ts = []
    for _ in range(a.iters):
        t = time.perf_counter(); fn(); torch.cuda.synchronize(); ts.append(time.perf_counter() - t)
    return round(statistics.median(ts) * 1e3, 3), round(min(ts) * 1e3, 3)


def key_and_proofs(n, ell, seed):
    u = ints(inputs.random_scalars(ell + 1, seed=seed))
    x = np.ascontiguousarray(inputs.random_scalars(n * ell, seed=seed + 1).reshape(n, ell, 4))
    xi = [ints(row) for row in x]
    av, bv = ints(inputs.random_scalars(n, seed=seed + 2)), ints(inputs.random_scalars(n, seed=seed + 3))
    dinv = pow(DELTA, -1, R)
    cv = [(av[i] * bv[i] - ALPHA * BETA - GAMMA * (u[0] + sum(p * q for p, q in zip(xi[i], u[1:])))) * dinv % R for i in range(n)]
    g1, g2 = mul(1, [ALPHA] + u).cpu().numpy().view(np.uint64), mul(2, [BETA, GAMMA, DELTA]).cpu().numpy().view(np.uint64)
    vk = {"alpha_g1": g1[0].copy(), "beta_g2": g2[0].copy(), "gamma_g2": g2[1].copy(), "delta_g2": g2[2].copy(), "ic": np.ascontiguousarray(g1[1:])}
    return zk.pairing.prepare_verifying_key_dev(vk), (mul(1, av), mul(2, bv), mul(1, cv)), x, xi


print(json.dumps({"device": torch.cuda.get_device_name(0), "lane_target": zk.lib.FIXED_BASES_LANE_TARGET}), flush=True)
for lg in [int(v) for v in a.sizes.split(",") if v]:
    for ell in [int(v) for v in a.inputs.split(",") if v]:
        n = 1 << lg
        pvk, (pa, pb, pc), x, xi = key_and_proofs(n, ell, 7000 + 10 * lg + ell)
        d_x = torch.from_numpy(x.view(np.int64)).cuda()
        m = min(n, a.baseline_max)
        ha, hb, hc = (t[:m].cpu().numpy().view(np.uint64) for t in (pa, pb, pc))
        plist = [(ha[i], hb[i], hc[i]) for i in range(m)]
        t = time.perf_counter(); base = zk.pairing.verify_proofs(pvk, plist, xi[:m]); t_base = (time.perf_counter() - t) * 1e3
        res = [None, None]

        def run_dev(): res[0] = zk.pairing.verify_proofs_dev(pvk, (pa, pb, pc), d_x)
        def run_batch(): res[1] = zk.pairing.verify_proofs_batch(pvk, (pa, pb, pc), d_x, key=KEY)
        def run_batch_unchecked(): zk.pairing.verify_proofs_batch(pvk, (pa, pb, pc), d_x, key=KEY, check_g2_subgroup=False)
        def run_acc(): zk.pairing.input_accumulators(pvk, d_x)
        pairs = zk.pairing.batch_pairs(pvk, (pa, pb, pc), d_x, KEY)
        one_group = torch.tensor([0, n + 3], dtype=torch.int32, device="cuda")
        def run_pairs(): zk.pairing.batch_pairs(pvk, (pa, pb, pc), d_x, KEY)
        def run_product(): zk.pairing.pairing_product(pairs[0], pairs[1], one_group)
        tabs = [zk.FixedBaseTable(pvk["ic"][j + 1]) for j in range(ell)]
        cols = [d_x[:, j].contiguous() for j in range(ell)]
        def run_single():
            for tab, col in zip(tabs, cols): tab.mul(col)
        dev_ms, batch_ms, unchecked_ms, acc_ms, single_ms = timed(run_dev), timed(run_batch), timed(run_batch_unchecked), timed(run_acc), timed(run_single)
        pairs_ms, product_ms = timed(run_pairs), timed(run_product)
        print(json.dumps({"log_n": lg, "inputs": ell, "baseline_proofs_timed": m, "baseline_ms_scaled_to_n": round(t_base * n / m, 1), "baseline_is_prefix": m < n,
                          "verify_proofs_dev_ms": dev_ms[0], "verify_proofs_dev_min_ms": dev_ms[1], "verify_proofs_batch_ms": batch_ms[0],
                          "verify_proofs_batch_min_ms": batch_ms[1], "verify_proofs_batch_no_subgroup_check_ms": unchecked_ms[0], "batch_pairs_ms": pairs_ms[0], "batch_product_one_group_ms": product_ms[0],
                          "lincomb_ms": acc_ms[0], "lincomb_min_ms": acc_ms[1], "fixed_base_mul_per_input_ms": single_ms[0],
                          "verdicts_ok": bool(base.all() and res[0].all() and res[1] is True)}), flush=True)

# the slice plan: rows x bases under forced slice lengths (0 = the plan)
for shape in [s for s in a.plan_shapes.split(",") if s]:
    n, n_bases = (int(v) for v in shape.split("x"))
    tab = zk.pairing.FixedBasesTable(mul(1, ints(inputs.random_scalars(n_bases, seed=7900))).cpu().numpy().view(np.uint64))
    d_k = torch.from_numpy(np.ascontiguousarray(inputs.random_scalars(n * n_bases, seed=7901).reshape(n, n_bases, 4)).view(np.int64)).cuda()
    sl, ns = C.c_size_t(0), C.c_size_t(0)
    assert L.mi355zk_fixed_bases_plan(n, n_bases, C.byref(sl), C.byref(ns)) == 0
    row, ref = {"rows": n, "bases": n_bases, "planned_slice_len": sl.value, "planned_slices": ns.value}, None
    for v in [s for s in a.plan_slices.split(",") if s]:
        slice_len = n_bases if v == "all" else int(v)
        if slice_len > n_bases: continue
        out = [None]
        def run(): out[0] = tab.lincomb(d_k, None, slice_len)
        row["slice_len_%s_ms" % v] = timed(run)[0]
        ref = out[0] if ref is None else ref
        assert torch.equal(out[0], ref), (shape, v)
    print(json.dumps(row), flush=True)
