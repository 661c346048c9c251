"""Child process of test_gpu_bases_cache.py: LRU eviction of the pinned-bases cache at its capacity.  The parent sets
MI355ZK_BASES_CACHE_GB=0.0006 (644 245 bytes; the capacity is read once per process): the device copy of a pinned G1 vector of 4096 points is
262 144 bytes, so two vectors fit and three do not.  Every multiexp is checked against the CPU oracle; after every step the cache is asked
(mi355zk_bases_cache_info) what it holds of each vector.  Prints one JSON line: per step the oracle comparison and the device bytes of
A, B, C and D (None: not found), or the text of the exception the call raised; stops at the first exception."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import inputs
import oracle_lib as O
import phase2_bn254_amd as zk

N, N_BIG = 1 << 12, 1 << 14
worker = zk.Worker(0)
L = zk.lib.load()
scalars = inputs.random_scalars(N, seed=4100)
# (contiguous u64 records: the calls below pass these very arrays, whose addresses are what was pinned)
vec = {name: np.ascontiguousarray(inputs.bases_progression_cpu(1, N_BIG if name == "D" else N, seed=4101 + i), dtype=np.uint64) for i, name in enumerate("ABCD")}
want = {}
for name, bases in vec.items():   # (every expected point before the first call on the device)
    rc, w = O.G1.multiexp(bases[:N], scalars, threads=8)
    assert rc == 0
    want[name] = O.G1.to_affine(w)
    zk.pin_bases(bases)


def held():
    out = {}
    for name, bases in vec.items():
        d, t = C.c_size_t(0), C.c_size_t(0)
        found = L.mi355zk_bases_cache_info(bases.ctypes.data_as(C.c_void_p), C.byref(d), C.byref(t))
        assert t.value == 0 and (found == 1 or d.value == 0)
        out[name] = d.value if found else None
    return out


out = {}
for step in ("A", "B", "C", "B again", "A again", "D"):
    name = step[0]
    try:
        got = zk.multiexp(worker, (vec[name], 0), zk.FullDensity(), scalars).wait()
    except Exception as e:  # reported, not raised: the parent shows which step it was
        out[step] = "%s: %s" % (type(e).__name__, e)
        break
    out[step] = [bool(np.array_equal(O.G1.to_affine(got), want[name])), held()]
else:
    L.mi355zk_bases_cache_invalidate(None)
    out["invalidate"] = [True, held()]
print(json.dumps(out))
