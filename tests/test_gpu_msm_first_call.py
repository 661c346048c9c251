"""The LDS limits of the multiexp's kernels are raised on first use, and the kernels of the group-independent stages (msm_partition.hip) are
shared by G1 and G2: whichever group calls first in a process configures them for both (part_configure(dev)), and each group still has to
configure its own tree kernel (part_configure<F>).  tests/msm_first_call_check.py runs in a fresh child process per order -- G2 then G1,
and G1 then G2 -- with two sizes per group:

  n = 4096   the G2 tree kernel always asks for 72 KiB of LDS, above the 64 KiB a kernel gets without asking; against the CPU oracle
  n = 2^17   the smallest power of two at which the plan's scatter launch asks for more than 64 KiB: msm_plan() gives st = 8192, nbin = 16,
             (2 * 16 + 32) * 4 + 8192 * 8 = 65 792 B for both groups (2^16: st = 4096, 32 960 B -- `test_msm_host dump` shows that row and the
             132 224 B of 2^20; the powers of two in between were read from the same msm_plan()); against the closed form (sum s_i k_i) * G
             over bases k_i * G, as test_gpu_msm.py::test_g2_msm_at_2e20_closed_form does

A kernel left unconfigured shows up as a refused launch (the call returns a device error, which the child reports as text), not as a
fault."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ORDERS = ("21", "12")
LIMIT = 120  # seconds per child; one takes a few


@pytest.fixture(scope="module")
def children():
    """Both children side by side (two processes on the one GPU), each under its own time limit."""
    here = os.path.dirname(os.path.abspath(__file__))
    procs = {o: subprocess.Popen([sys.executable, os.path.join(here, "msm_first_call_check.py"), o], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
             for o in ORDERS}
    res = {}
    for o, p in procs.items():
        try:
            out, err = p.communicate(timeout=LIMIT)
        except subprocess.TimeoutExpired:
            p.kill()
            out, err = p.communicate()
            err += "\n(killed after %d s)" % LIMIT
        res[o] = (p.returncode, out, err)
    return res


@pytest.mark.parametrize("order", ORDERS)
def test_first_multiexp_of_the_process(children, order):
    rc, out, err = children[order]
    assert rc == 0, (out[-2000:], err[-4000:])
    got = json.loads(out.strip().splitlines()[-1])
    want = {"g%s n=%d" % (g, n): True for g in order for n in (1 << 12, 1 << 17)}
    assert got == want
    assert list(got) == list(want)  # (the steps ran in this order)
