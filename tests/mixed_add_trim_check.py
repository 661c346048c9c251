"""Child process of tests/test_gpu_mixed_add_trim.py.  The library reads its knobs once per process, so the parent starts this interpreter with
MI355ZK_G1_PAIR=0, MI355ZK_MSM_SPLIT=0 and MI355ZK_MSM_C=6: every G1 call runs one lane per bucket (msm_accumulate_kernel /
msm_accumulate_heavy_kernel -> accumulate_run -> xyzzu_add_mixed) over windows of 32 buckets, so that 2^12 points put more than a hundred entries of
both signs into every bucket and the bucket reduction (xyzzr_add) adds full records.  Every case is compared by affine point with the CPU oracle's
multiexp; one JSON line {case: {"ok": bool, ...}} leaves on stdout."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import bn254_model as M
import inputs
import oracle_lib as O
import phase2_bn254_amd as zk

assert os.environ.get("MI355ZK_G1_PAIR") == "0" and os.environ.get("MI355ZK_MSM_SPLIT") == "0" and os.environ.get("MI355ZK_MSM_C") == "6"
os.environ.pop("MI355ZK_HOST_CHUNK_TEST", None)
G = O.G1
L = zk.lib.load()
worker = zk.Worker(0)
geom = np.zeros(5 + 128, np.uint32)
assert L.mi355zk_selftest_msm_digits(4096, 1, None, 0, 0, 0, None, geom.ctypes.data) == 0
assert int(geom[0]) == 6 and int(geom[2]) == 32, [int(x) for x in geom[:6]]          # c = 6: 32 signed buckets per window

POOL = inputs.bases_progression_cpu(1, 1 << 14, seed=9101)
out = {}


def neg(b):
    y = sum(int(v) << (64 * i) for i, v in enumerate(b[4:]))
    o = b.copy()
    o[4:] = M.to_limbs(M.Q - y)
    return o


def run_plain(bases, scalars):
    return G.to_affine(zk.multiexp(worker, (bases, 0), zk.FullDensity(), scalars).wait())


def oracle(bases, scalars):
    rc, want = G.multiexp(bases, scalars, threads=4)
    assert rc == 0, rc
    return G.to_affine(want)


def launches(bases, scalars):
    L.mi355zk_prof_reset()
    L.mi355zk_prof_enable(1)
    try:
        zk.multiexp(worker, (bases, 0), zk.FullDensity(), scalars).wait()
    finally:
        L.mi355zk_prof_enable(0)
    res = {}
    for name in ("msm_accumulate", "msm_accumulate_heavy"):
        tot, cnt = C.c_double(), C.c_long()
        L.mi355zk_prof_get(name.encode(), C.byref(tot), C.byref(cnt))
        res[name] = (tot.value, cnt.value)
    return res


def check(name, bases, scalars, path=None):
    bases, scalars = np.ascontiguousarray(bases.astype(np.uint64)), np.ascontiguousarray(scalars.astype(np.uint64))
    out[name] = {"ok": bool(np.array_equal(run_plain(bases, scalars), oracle(bases, scalars))), "n": len(bases)}
    if path is not None:
        seen = launches(bases, scalars)
        out[name]["launches"] = seen
        out[name]["ok"] = out[name]["ok"] and bool(path(seen))


# 2^12 and 2^14 points, random 254-bit exponents: every bucket of every window holds ~128 / ~512 entries of both signs
check("2^12 points", POOL[:1 << 12], inputs.random_scalars(1 << 12, seed=9201))
check("2^14 points", POOL, inputs.random_scalars(1 << 14, seed=9202))

# repeated bases: every base four times in a row under ONE exponent (P + P on the second entry of a bucket, 2P + P, ...), and a negated copy
# under the same exponent further on (P - P inside the bucket whenever the running sum is that point)
k = 256
sc = inputs.random_scalars(k, seed=9203)
b = np.concatenate([np.repeat(POOL[:k], 4, axis=0), np.stack([neg(p) for p in POOL[:k]]), POOL[k:k + 64], np.stack([neg(p) for p in POOL[k:k + 64]])])
s = np.concatenate([np.repeat(sc, 4, axis=0), sc, np.tile(np.array([[5, 0, 0, 0]], np.uint64), (128, 1))])      # the last 128: P_i then -P_i, all in bucket 5 of window 0
check("repeated and negated bases", b, s)
b2 = np.stack([POOL[0], POOL[0], neg(POOL[1]), neg(POOL[1]), POOL[2], neg(POOL[2]), POOL[3]])
s2 = np.array([[3, 0, 0, 0]] * 4 + [[4, 0, 0, 0]] * 2 + [[9, 0, 0, 0]], np.uint64)                                 # P + P; -Q - Q; P - P; a one-entry run
check("P + P, -Q - Q, P - P and a one-entry run", b2, s2)

# one-entry runs: 31 points, 31 different digits of window 0
check("one-entry runs", POOL[100:131], np.array([[d + 1, 0, 0, 0] for d in range(31)], np.uint64))

# identity records among the entries, dense mode (they add nothing)
import torch

dev = torch.device("cuda", 0)
n = 1 << 10
b = POOL[:n].copy()
b[::7] = 0
s = inputs.random_scalars(n, seed=9204)
d_b = torch.from_numpy(np.ascontiguousarray(b).view(np.int64)).to(dev)
d_s = torch.from_numpy(np.ascontiguousarray(s).view(np.int64)).to(dev)
res = np.zeros(12, np.uint64)
rc = L.mi355zk_bn254_g1_dense_multiexp_dev(C.c_void_p(d_b.data_ptr()), C.c_void_p(d_s.data_ptr()), n, None, res.ctypes.data_as(C.c_void_p))
s_o = s.copy()
s_o[~b.any(axis=1)] = 0
out["identity records, dense"] = {"ok": rc == 0 and bool(np.array_equal(G.to_affine(res), oracle(b, s_o))), "n": n}

# the bucket array of one 2^12 call, word for word: the records the accumulate stage left (before the reduction) against the records the formulas had
# BEFORE the addition was trimmed -- the same buckets, from the index lists this very call reports, accumulated by the big-int model of those formulas
# (mixed_add_trim_vectors.bucket_record: the pair start, then mixed additions in list order; a record's coordinates are canonical, so they depend on the
# sequence of group-law formulas and on nothing else).  The reference is computed per call and not stored: the partition does not leave a bucket's entries in
# the same order from run to run, and with the order goes the Z of every record.
def bucket_array(bases, scalars):
    n = len(bases)
    d_b = torch.from_numpy(np.ascontiguousarray(bases.astype(np.uint64)).view(np.int64)).to(dev)
    d_s = torch.from_numpy(np.ascontiguousarray(scalars.astype(np.uint64)).view(np.int64)).to(dev)
    res, cnt = np.zeros(12, np.uint64), np.zeros(2, np.uint32)
    cap_b, cap_v = 1 << 13, 1 << 19
    first, last, vals, rec = np.zeros(cap_b, np.uint32), np.zeros(cap_b, np.uint32), np.zeros(cap_v, np.uint32), np.zeros((cap_b, 16), np.uint64)
    rc = L.mi355zk_selftest_g1_msm_buckets_dev(C.c_void_p(d_b.data_ptr()), C.c_void_p(d_s.data_ptr()), n, None, res.ctypes.data, cnt.ctypes.data, cnt.ctypes.data + 4,
                                               first.ctypes.data, last.ctypes.data, cap_b, vals.ctypes.data, cap_v, rec.ctypes.data)
    assert rc == 0, (rc, cnt)
    nb, nv = int(cnt[0]), int(cnt[1])
    return res, first[:nb].copy(), last[:nb].copy(), vals[:nv].copy(), rec[:nb].copy()


BUCKET_N, BUCKET_SEED = 1 << 12, 9207
b = np.ascontiguousarray(POOL[:BUCKET_N].astype(np.uint64))
s = inputs.random_scalars(BUCKET_N, seed=BUCKET_SEED)
res, first, last, vals, rec = bucket_array(b, s)
sizes = (last - first).astype(np.int64)
signs = vals[np.concatenate([np.arange(f, l) for f, l in zip(first, last)])] >> 31
import mixed_add_trim_vectors as TV

_pts = []
for row in b:
    x, y = (sum(int(w) << (64 * i) for i, w in enumerate(half)) * TV.I256 % M.Q for half in (row[:4], row[4:]))
    _pts.append((x, y))
gold = np.array([TV.bucket_record([(_pts[int(v) & 0x7FFFFFFF][0], (M.Q - _pts[int(v) & 0x7FFFFFFF][1]) % M.Q if int(v) >> 31 else _pts[int(v) & 0x7FFFFFFF][1])
                                   for v in vals[f:l]]) for f, l in zip(first, last)], dtype=np.uint64).reshape(-1, 16)
# A bucket longer than the planner's heavy limit (msm_plan.hpp: 2 * mean + 16 for a call this short; here the few buckets of the short top window) is summed
# by the segment-parallel path, in another order of additions: the same point under another Z.  Those are compared as points, every other record word for word.
heavy = 2 * (int(sizes.sum()) // len(sizes) + 1) + 16
light = sizes <= heavy


def coord(r, k):
    return sum(int(w) << (64 * i) for i, w in enumerate(r[4 * k:4 * k + 4]))


def same_point(r, g):
    if not r.any() or not g.any():
        return not r.any() and not g.any()
    return (coord(r, 0) * coord(g, 2) - coord(g, 0) * coord(r, 2)) % M.Q == 0 and (coord(r, 1) * coord(g, 3) - coord(g, 1) * coord(r, 3)) % M.Q == 0


shape_ok = gold.shape == rec.shape
out["bucket array, word for word"] = {
    "ok": bool(shape_ok and np.array_equal(rec[light], gold[light]) and all(same_point(rec[i], gold[i]) for i in np.nonzero(~light)[0])
               and int((~light).sum()) <= len(rec) // 100 and np.array_equal(G.to_affine(res), oracle(b, s))
               and int(sizes.sum()) > 40 * BUCKET_N and int((sizes >= 4).sum()) > 0.9 * len(sizes) and 0.3 < float(signs.mean()) < 0.7 and rec.any(axis=1).sum() > 0.9 * len(rec)),
    "buckets": int(len(rec)), "entries": int(sizes.sum()), "heavy buckets": int((~light).sum()),
    "differing records": int((rec[light] != gold[light]).any(axis=1).sum()) if shape_ok else -1}
# skewed: three quarters of the exponents are 1 (the 0/1 witnesses of a prover): bucket 1 of window 0 takes the heavy path
n = 1 << 12
s = inputs.random_scalars(n, seed=9205)
s[np.arange(n) % 4 != 0] = np.array([1, 0, 0, 0], np.uint64)
check("skewed exponents, the heavy path", POOL[:n], s, path=lambda seen: seen["msm_accumulate_heavy"][1] >= 1)

# a streamed host-buffer call in three chunks: the CARRY instantiation takes every bucket's record up again
os.environ["MI355ZK_HOST_CHUNK_TEST"] = "1024"
n = 3 * 1024
s = inputs.random_scalars(n, seed=9206)
b = np.ascontiguousarray(POOL[:n].astype(np.uint64))
seen = launches(b, s)
same = bool(np.array_equal(run_plain(b, s), oracle(b, s)))
out["streamed, three chunks"] = {"ok": same and seen["msm_accumulate"][1] == 3, "same": same, "n": n, "launches": seen}
os.environ.pop("MI355ZK_HOST_CHUNK_TEST")
print(json.dumps(out))
