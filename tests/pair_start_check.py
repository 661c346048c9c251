"""Child process of tests/test_gpu_msm_pair_start.py.  The library reads MI355ZK_G1_PAIR and MI355ZK_MSM_C once per process, so the parent
starts this interpreter with MI355ZK_G1_PAIR=0, MI355ZK_MSM_SPLIT=0 and MI355ZK_MSM_C=10: every G1 call then runs one lane per bucket
(msm_accumulate_kernel / msm_accumulate_heavy_kernel -> accumulate_run) over 26 windows of 512 buckets, and an exponent below 512 is one
positive digit of window 0 -- the points that share it are one bucket, in index order.  Every case is compared exactly (affine words)
with the CPU oracle's multiexp; one JSON line {case: {"ok": bool, ...}} leaves on stdout.  n <= 4096 throughout."""
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

assert os.environ.get("MI355ZK_G1_PAIR") == "0" and os.environ.get("MI355ZK_MSM_SPLIT") == "0" and os.environ.get("MI355ZK_MSM_C") == "10"
os.environ.pop("MI355ZK_HOST_CHUNK_TEST", None)
G = O.G1
L = zk.lib.load()
worker = zk.Worker(0)
geom = np.zeros(5 + 128, np.uint32)
assert L.mi355zk_selftest_msm_digits(4096, 1, None, 0, 0, 0, None, geom.ctypes.data) == 0
c, W, nb, rmul = (int(x) for x in geom[:4])
width0 = int(geom[5])
assert (c, nb, rmul, width0) == (10, 512, 1, 10), (c, W, nb, rmul, width0)
B0 = 1 << width0                                   # exponent B0 - d: digit -d in window 0 and a carry into window 1

POOL = inputs.bases_progression_cpu(1, 4096, seed=8101)
_next = [0]


def fresh(k=1):
    """k bases no case has used yet"""
    i = _next[0]
    _next[0] += k
    assert _next[0] <= len(POOL)
    return [POOL[j].copy() for j in range(i, i + k)]


def neg(b):
    y = sum(int(v) << (64 * i) for i, v in enumerate(b[4:]))
    out = b.copy()
    out[4:] = M.to_limbs(M.Q - y)                  # -(y R) = (-y) R  (mod q): the Montgomery form of -y
    return out


def small(d):
    return [int(d), 0, 0, 0]


def arrays(entries):
    """[(base, exponent limbs)] -> bases [n, 8], scalars [n, 4]"""
    return (np.ascontiguousarray(np.stack([b for b, _ in entries]).astype(np.uint64)),
            np.ascontiguousarray(np.array([s for _, s in entries], dtype=np.uint64).reshape(len(entries), 4)))


def run_plain(bases, scalars):
    return G.to_affine(zk.multiexp(worker, (bases, 0), zk.FullDensity(), scalars).wait())


def oracle(bases, scalars):
    rc, want = G.multiexp(bases, scalars, threads=4)
    assert rc == 0, rc
    return G.to_affine(want)


def launches(bases, scalars):
    """the same call again under the library's per-group HIP-event timing: {group: (ms, event records = launches of the group)}"""
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


out = {}


def check(name, entries, path=None):
    """path: None, or a predicate over launches() that shows the call took the path the case is about"""
    bases, scalars = arrays(entries)
    assert len(bases) <= 4096
    got, want = run_plain(bases, scalars), oracle(bases, scalars)
    out[name] = {"ok": bool(np.array_equal(got, want)), "n": len(bases)}
    if path is not None:
        seen = launches(bases, scalars)
        out[name]["launches"] = seen
        out[name]["ok"] = out[name]["ok"] and bool(path(seen))


def buckets(groups, digits=None):
    """groups: lists of bases, one list per bucket; bucket g gets the digit digits[g] (default g + 1).  The entries are interleaved round-robin, so a
    bucket's points are spread over the index range and keep their order inside the bucket."""
    entries = []
    depth = max(len(g) for g in groups)
    for k in range(depth):
        for g, pts in enumerate(groups):
            if k < len(pts):
                entries.append((pts[k], small(digits[g] if digits else g + 1)))
    return entries


# ---- bucket lengths: the 4-entry index groups and their boundaries (1, 2, 3 | 4, 5 | 8, 9), eight buckets of each length
SIZES = (1, 2, 3, 4, 5, 8, 9)
check("sizes window 0", buckets([fresh(k) for k in SIZES for _ in range(8)]), path=lambda seen: seen["msm_accumulate"][1] == 1)   # one chunk, one launch
# the same lengths in EVERY window: sixteen random 254-bit exponents per length, each shared by k points (signed digits of both signs)
entries = []
for k in SIZES:
    for s in inputs.random_scalars(16, seed=8200 + k):
        entries += [(b, [int(v) for v in s]) for b in fresh(k)]
order = np.random.default_rng(8201).permutation(len(entries))
check("sizes every window", [entries[i] for i in order])

# ---- the bucket opens with P, P under the same digit: a doubling, then 0, 1 and 3 further points
for more in (0, 1, 3):
    groups = []
    for _ in range(6):
        p = fresh()[0]
        groups.append([p, p.copy()] + fresh(more))
    check("doubling then %d" % more, buckets(groups))
p = fresh()[0]
check("the same point nine times", buckets([[p.copy() for _ in range(9)], fresh(2)]))

# ---- the bucket opens with a pair that cancels, then 0, 1 and 2 further points: by a negated base, and by opposite signed digits
for more in (0, 1, 2):
    groups = []
    for _ in range(6):
        p = fresh()[0]
        groups.append([p, neg(p)] + fresh(more))
    check("cancel by negated base then %d" % more, buckets(groups))
    entries = []
    for g in range(6):
        p, d = fresh()[0], g + 1
        entries.append((p, small(d)))
        entries.append((p.copy(), small(B0 - d)))          # digit -d: the same bucket with the sign bit; the carry goes to window 1
        entries += [(q, small(d)) for q in fresh(more)]
    check("cancel by opposite digits then %d" % more, entries)
p, q = fresh(2)
check("P, -P, Q, -Q: the all-zero record", buckets([[p, neg(p), q, neg(q)], fresh(3), [p.copy(), neg(p), q.copy(), neg(q), fresh()[0]]]))

# ---- the identity record as the first and as the second entry of a bucket
import torch

dev = torch.device("cuda", 0)


def run_dense(bases, scalars):
    d_b = torch.from_numpy(bases.view(np.int64)).to(dev)
    d_s = torch.from_numpy(scalars.view(np.int64)).to(dev)
    res = np.zeros(12, np.uint64)
    assert L.mi355zk_bn254_g1_dense_multiexp_dev(C.c_void_p(d_b.data_ptr()), C.c_void_p(d_s.data_ptr()), len(bases), None, res.ctypes.data_as(C.c_void_p)) == 0
    return G.to_affine(res)


zero = np.zeros(8, np.uint64)
for where in ("first", "second", "first and second"):
    groups = []
    for g in range(5):
        pts = fresh(2 + g)                               # buckets of 2 .. 6 entries
        if "first" in where:
            pts[0] = zero.copy()
        if "second" in where:
            pts[1] = zero.copy()
        groups.append(pts)
    groups.append(fresh(4))
    bases, scalars = arrays(buckets(groups))
    dense_sc = scalars.copy()
    dense_sc[~bases.any(axis=1)] = 0                     # dense semantics: an identity base adds nothing
    out["identity %s, dense" % where] = {"ok": bool(np.array_equal(run_dense(bases, scalars), oracle(bases, dense_sc)))}
    lowest = int(np.nonzero(~bases.any(axis=1))[0][0])
    rc_o, _ = G.multiexp(bases, scalars, threads=1)
    try:
        zk.multiexp(worker, (bases, 0), zk.FullDensity(), scalars).wait()
        res = {"ok": False, "error": "none"}
    except zk.SynthesisError as e:
        res = {"ok": e.kind == zk.SynthesisError.UNEXPECTED_IDENTITY and e.index == lowest and rc_o == 1, "kind": str(e.kind), "index": int(e.index), "lowest": lowest}
    out["identity %s, plain" % where] = res

# ---- one bucket holds every point (all exponents equal): the heavy path, 64 strided lanes per segment of 128 entries.  Entries j and j + 64 of a
# segment are one lane's run: made equal (the lane opens with a doubling) and opposite (with a pair that cancels), in both full segments
for name, expo in (("window 0", small(7)), ("every window", [int(v) for v in inputs.random_scalars(1, seed=8300)[0]])):
    pts = fresh(300)
    for j, what in ((3, "same"), (10, "opposite"), (128 + 5, "same"), (128 + 63, "opposite"), (0, "opposite"), (128 + 0, "same")):
        pts[j + 64] = pts[j].copy() if what == "same" else neg(pts[j])
    # That the bucket really left the lane-per-bucket launch: one lane walking its 300 entries is 299 dependent additions of ~8 us each whatever else
    # the device does (msm_plan.hpp: the reason the heavy path exists), 2.4 ms; with the bucket cut into 64-lane segments the launch holds nothing
    # longer than the (empty) other buckets and lasts some tens of microseconds.  A third of the serial walk separates the two by a wide margin.
    check("heavy bucket, " + name, [(b, expo) for b in pts], path=lambda seen: seen["msm_accumulate_heavy"][1] >= 1 and seen["msm_accumulate"][0] < 0.8)

# ---- a streamed host-buffer call in four chunks of 64 exponents (chunk 0 opens its buckets with the pair start, the three CARRY launches keep the
# loop and take up what it left): digit 1 is touched in every chunk (twice and more), digit 2
# in chunk 1 only, digit 3 once in chunk 2, digit 4 cancels in chunk 0 and is taken up again by chunks 1 and 3 (a carried record that is
# infinity), digit 5 doubles across the chunk boundary; the other 507 buckets of window 0 and the other windows stay empty
os.environ["MI355ZK_HOST_CHUNK_TEST"] = "64"
n = 256
pts = fresh(n)
digs = [1] * n
for i in range(n):
    digs[i] = 1 if i % 5 else 6 + i % 3                  # digits 6, 7, 8: ordinary buckets touched in every chunk
for i in (64 + 3, 64 + 9, 64 + 30):
    digs[i] = 2
digs[128 + 17] = 3
pts[7] = neg(pts[2])
for i in (2, 7, 64 + 11, 64 + 12, 192 + 1, 192 + 40, 192 + 41):
    digs[i] = 4
pts[64 + 21] = pts[33].copy()
pts[64 + 22] = pts[33].copy()
for i in (33, 64 + 21, 64 + 22):
    digs[i] = 5
bases, scalars = arrays([(b, small(d)) for b, d in zip(pts, digs)])
four = lambda seen: seen["msm_accumulate"][1] == 4            # one lane-per-bucket launch per chunk: the first fresh, three CARRY
seen = launches(bases, scalars)
out["streamed, four chunks"] = {"ok": bool(np.array_equal(run_plain(bases, scalars), oracle(bases, scalars))) and four(seen), "n": n, "launches": seen}
sc = inputs.random_scalars(n, seed=8400)
seen = launches(bases, sc)
out["streamed, four chunks, random exponents"] = {"ok": bool(np.array_equal(run_plain(bases, sc), oracle(bases, sc))) and four(seen), "n": n, "launches": seen}
os.environ.pop("MI355ZK_HOST_CHUNK_TEST")
out["bases used"] = {"ok": _next[0] <= 4096, "n": _next[0]}
print(json.dumps(out))
