#!/usr/bin/env python3
"""Many proofs over one Parameters: the batched multiexp (bellman.multiexp_many = mi355zk_bn254_g{1,2}_msm_batch_dev) against a loop of
multiexp, and prover.create_proofs against a loop of create_proof, on one MI355X with the data resident in HBM.

  multiexp   G1 and G2, n = 2^12, 2^16, 2^20, B = 1, 4, 16: ms per BATCH for both arms and the ratio loop / batch
  proofs     2^16 and 2^20 constraints, B = 16 (synthetic instance of tools/bench_prover.py, B witnesses): ms per batch of proofs

Both arms run in this process, alternating (loop, batch, loop, batch, ...) after every shape has been warmed up (code objects, workspace pools,
pinned buffers, the prover's threads and streams); the figure is the median of --iters rounds, the minimum beside it.  Results are compared
before they are timed: a batch that is faster and different is not faster.  Prints one JSON line; --markdown writes the table of
profiles/prove_batch.md."""
import argparse, ctypes as C, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import phase2_bn254_amd as zk, inputs, bench, oracle_lib as O

ap = argparse.ArgumentParser()
ap.add_argument("--iters", type=int, default=9)
ap.add_argument("--sizes", default="12,16,20"); ap.add_argument("--batches", default="1,4,16")
ap.add_argument("--proof-sizes", default="16,20"); ap.add_argument("--proof-batch", type=int, default=16)
ap.add_argument("--markdown", default=None)
a = ap.parse_args()
L = zk.lib.load(); w = zk.Worker(0); dev = torch.device("cuda", 0)

def synth(group, n, seed):
    k = bench.gen_scalars(n, seed, dev); p = torch.empty((n, 8 * group), dtype=torch.int64, device=dev)
    gen = np.ascontiguousarray(inputs.G1_GEN_RAW if group == 1 else inputs.G2_GEN_RAW)
    fn = L.mi355zk_bn254_g1_batch_mul_dev if group == 1 else L.mi355zk_bn254_g2_batch_mul_dev
    assert fn(C.c_void_p(p.data_ptr()), gen.ctypes.data_as(C.c_void_p), C.c_void_p(k.data_ptr()), n, None) == 0
    return p

def affine(jac):
    jac = np.ascontiguousarray(jac, dtype=np.uint64); out = np.zeros(jac.size // 12 * 8, dtype=np.uint64)
    fn = L.mi355zk_bn254_g1_to_affine if jac.size == 12 else L.mi355zk_bn254_g2_to_affine
    assert fn(out.ctypes.data_as(C.c_void_p), jac.ctypes.data_as(C.c_void_p)) == 0
    return out

def alternate(arms, iters):
    """{name: (median ms, min ms)} of the arms run in turn, `iters` rounds"""
    ts = {k: [] for k in arms}
    for _ in range(iters):
        for k, fn in arms.items():
            t = time.perf_counter(); fn(); torch.cuda.synchronize(); ts[k].append((time.perf_counter() - t) * 1e3)
    return {k: (sorted(v)[len(v) // 2], min(v)) for k, v in ts.items()}

rows, proof_rows = [], []
for group in (1, 2):
    for lg in [int(x) for x in a.sizes.split(",") if x]:
        n = 1 << lg
        bases = synth(group, n, 100 + group)
        for B in [int(x) for x in a.batches.split(",") if x]:
            sc = bench.gen_scalars(B * n, 200 + lg + B, dev).reshape(B, n, 4).contiguous()   # Montgomery Fr, as the prover holds them
            vecs = [sc[v] for v in range(B)]
            loop = lambda: [zk.multiexp(w, (bases, 0), zk.FullDensity(), v, scalars_montgomery=True).wait() for v in vecs]
            batch = lambda: [f.wait() for f in zk.multiexp_many(w, (bases, 0), zk.FullDensity(), sc, scalars_montgomery=True)]
            for _ in range(3): want, got = loop(), batch()
            assert all(np.array_equal(affine(x), affine(y)) for x, y in zip(want, got)), ("results differ", group, lg, B)
            torch.cuda.synchronize()
            t = alternate({"loop": loop, "batch": batch}, a.iters)
            rows.append({"group": group, "log_n": lg, "B": B, "loop_ms": round(t["loop"][0], 3), "batch_ms": round(t["batch"][0], 3),
                         "loop_min_ms": round(t["loop"][1], 3), "batch_min_ms": round(t["batch"][1], 3), "ratio": round(t["loop"][0] / t["batch"][0], 2)})
            del sc, vecs
        del bases; torch.cuda.empty_cache()

def witness(n, seed):  # Montgomery Fr with the 0 / 1 mix of a real witness (tools/bench_prover.py)
    v = bench.gen_scalars(n, seed, dev)
    g = torch.Generator(device=dev); g.manual_seed(seed + 1)
    kind = torch.randint(0, 10, (n,), device=dev, generator=g)
    one_m = torch.tensor([v_ - (1 << 64) if v_ >= (1 << 63) else v_ for v_ in [0xac96341c4ffffffb, 0x36fc76959f60cd29, 0x666ea36f7879462e, 0x0e0a77c19a07df2f]], dtype=torch.int64, device=dev)
    v[kind < 3] = 0; v[(kind >= 3) & (kind < 6)] = one_m
    return v

for lg in [int(x) for x in a.proof_sizes.split(",") if x]:
    B = a.proof_batch
    m = 1 << lg; num_inputs, num_aux = 16, m - 64
    rng = np.random.default_rng(1)
    a_bits, bi_bits, ba_bits = rng.random(num_aux) < 0.5, rng.random(num_inputs) < 0.5, rng.random(num_aux) < 0.4
    na, nb_ = int(a_bits.sum()), int(bi_bits.sum()) + int(ba_bits.sum())
    vk1 = O.G1.mul_many_affine(inputs.G1_GEN_RAW, inputs.random_scalars(3, seed=2)); vk2 = O.G2.mul_many_affine(inputs.G2_GEN_RAW, inputs.random_scalars(2, seed=3))
    vk = {"alpha_g1": vk1[0], "beta_g1": vk1[1], "delta_g1": vk1[2], "beta_g2": vk2[0], "delta_g2": vk2[1]}
    params = zk.prover.Parameters(vk, synth(1, m - 1, 10), synth(1, num_aux, 11), synth(1, num_inputs + na, 12), synth(1, nb_, 13), synth(2, nb_, 14))
    dens = [zk.DensityTracker.from_bools(x) for x in (a_bits, bi_bits, ba_bits)]
    asg = [zk.prover.ProvingAssignment(*[bench.gen_scalars(m, 20 + 10 * i + j, dev) for j in range(3)], witness(num_inputs, 30 + 10 * i), witness(num_aux, 31 + 10 * i), *dens)
           for i in range(B)]
    rs, ss = [12345 + i for i in range(B)], [67890 + 3 * i for i in range(B)]
    loop = lambda: [zk.prover.create_proof(w, params, p, r, s) for p, r, s in zip(asg, rs, ss)]
    batch = lambda: zk.prover.create_proofs(w, params, asg, rs, ss)
    for _ in range(2): want, got = loop(), batch()
    assert all(np.array_equal(x, y) for p, q in zip(want, got) for x, y in zip(p, q)), ("proofs differ", lg)
    torch.cuda.synchronize()
    t = alternate({"loop": loop, "batch": batch}, max(3, a.iters // 2))
    proof_rows.append({"log_m": lg, "B": B, "loop_ms": round(t["loop"][0], 2), "batch_ms": round(t["batch"][0], 2), "loop_min_ms": round(t["loop"][1], 2),
                       "batch_min_ms": round(t["batch"][1], 2), "ratio": round(t["loop"][0] / t["batch"][0], 2)})
    del params, asg; torch.cuda.empty_cache()

print(json.dumps({"device": torch.cuda.get_device_name(0), "iters": a.iters, "multiexp": rows, "proofs": proof_rows}))
if a.markdown:
    with open(a.markdown, "w") as f:
        f.write("| call | size | B | loop (ms) | batch (ms) | loop / batch |\n|---|---|---|---|---|---|\n")
        for r in rows:
            f.write("| G%d multiexp | 2^%d | %d | %.3f | %.3f | %.2f |\n" % (r["group"], r["log_n"], r["B"], r["loop_ms"], r["batch_ms"], r["ratio"]))
        for r in proof_rows:
            f.write("| create_proof | 2^%d | %d | %.2f | %.2f | %.2f |\n" % (r["log_m"], r["B"], r["loop_ms"], r["batch_ms"], r["ratio"]))
