"""Child process of test_gpu_msm_first_call.py.  argv[1] = the order of the groups, "21" (the first multiexp of the process is G2, then
G1) or "12".  For each group in that order: a 4096-point multiexp against the CPU oracle, then a 2^17-point multiexp over bases k_i * G
against the closed form (sum s_i k_i) * G.  Every input and every expected point is prepared BEFORE the first multiexp (batch_mul and the
oracle do not go through the multiexp's configuration), so the first multiexp really is the first group's.  Prints one JSON line: per
step True / False, or the text of the exception the call raised (a refused launch comes back as a DeviceError); stops at the first
exception."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

import bench
import bn254_model as M
import inputs
import oracle_lib as O
import phase2_bn254_amd as zk

SMALL, LARGE = 1 << 12, 1 << 17
order = [int(ch) for ch in sys.argv[1]]
assert sorted(order) == [1, 2]
worker = zk.Worker(0)
L = zk.lib.load()
dev = torch.device("cuda", 0)


def to_int(a):
    return sum(a[:, i].astype(object) << (64 * i) for i in range(4))


steps = []  # (label, bases, scalars, expected affine point)
for group in order:
    G = O.G1 if group == 1 else O.G2
    gen = np.ascontiguousarray(inputs.G1_GEN_RAW if group == 1 else inputs.G2_GEN_RAW)
    bases = inputs.bases_progression_cpu(group, SMALL, seed=3100 + group)
    scalars = inputs.random_scalars(SMALL, seed=3110 + group)
    rc, want = G.multiexp(bases, scalars, threads=8)
    assert rc == 0
    steps.append(("g%d n=%d" % (group, SMALL), bases, scalars, G.to_affine(want)))
    s = bench.gen_scalars(LARGE, 3120 + group, dev)
    k = bench.gen_scalars(LARGE, 3130 + group, dev)
    pts = torch.empty((LARGE, 8 * group), dtype=torch.int64, device=dev)
    mul = L.mi355zk_bn254_g1_batch_mul_dev if group == 1 else L.mi355zk_bn254_g2_batch_mul_dev
    assert mul(C.c_void_p(pts.data_ptr()), gen.ctypes.data_as(C.c_void_p), C.c_void_p(k.data_ptr()), LARGE, None) == 0
    torch.cuda.synchronize()
    hs, hk = s.cpu().numpy().view(np.uint64), k.cpu().numpy().view(np.uint64)
    dot = int(sum(int(a) * int(b) for a, b in zip(to_int(hs), to_int(hk))) % M.R_ORDER)
    steps.append(("g%d n=%d" % (group, LARGE), pts, s, G.to_affine(G.mul(G.from_affine(gen), M.to_limbs(dot)))))

out = {}
for label, bases, scalars, want in steps:
    G = O.G1 if label.startswith("g1") else O.G2
    try:
        got = zk.multiexp(worker, (bases, 0), zk.FullDensity(), scalars).wait()
    except Exception as e:  # reported, not raised: the parent shows which step it was
        out[label] = "%s: %s" % (type(e).__name__, e)
        break
    out[label] = bool(np.array_equal(G.to_affine(got), want))
print(json.dumps(out))
