"""Child process of tests/test_gpu_ntt_edges.py.  The library reads its knobs once per process, so the parent starts this interpreter with
MI355ZK_NTT_WAVELOCAL=0: the full tiles of a 2^20 transform then run the barrier radix-4 kernel (ntt_pass_kernel<10, true>) instead of the
wave-local one.  The four domain operations on a single tone (tests/ntt_edge_forms.py), byte for byte against the closed form; one JSON line
{op: {"ok": bool, ...}} leaves on stdout."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np

import ntt_edge_forms as E
import phase2_bn254_amd as zk

assert os.environ.get("MI355ZK_NTT_WAVELOCAL") == "0"
worker = zk.Worker(0)
LOG_N = 20
out = {}
for op in E.OPS:
    (name, a, want), = E.cases(LOG_N, op, which=["tone 1"])
    dom = zk.EvaluationDomain.from_coeffs(a)
    getattr(dom, op)(worker)
    got = dom.into_coeffs()
    bad = np.nonzero((got != want).any(axis=1))[0]
    out[op] = {"ok": len(bad) == 0, "pattern": name, "differing": int(len(bad)), "first": int(bad[0]) if len(bad) else None}
print(json.dumps(out))
