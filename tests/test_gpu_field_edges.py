"""The edge-operand table of tests/field_edge_vectors.py on the DEVICE: one primitive per lane through mi355zk_selftest_dev_op
(csrc/selftest_dev.hip), compared with Python big ints -- the gfx950 object code of field.hpp / fieldu.hpp / curveu.hpp, including what
exists in the device pass only: the inline-assembly Montgomery product and the quad- and pair-per-bucket additions.

  Fp, Fq2        equal to the big-int result, limb for limb
  FpU, Fq2U      congruent, value and limbs below the bound the source states, the exact integer where the op determines it; identical to
                 the host-compiled hook where one exists; the ZK_CHAIN_MAD build identical to the plain one
  group law      the normalised result is bn254_model's affine sum / double, infinity exactly where the model says; the records of the quad
                 and pair forms byte-identical to the one-lane result, in every lane of the group
No case is skipped or filtered: every row of every table is launched and checked (tests/test_field_edges_host.py shows the rows are inside
the contracts).  A failure names the op, the field, the class and the operand limbs."""
import numpy as np
import pytest

import bn254_model as M
import field_edge_vectors as V
from test_field_edges_host import _host_call

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib(zk, worker):
    return zk.lib.load()


def run(lib, op, which, rows, chain=False, lanes=1):
    """every row (each in `lanes` consecutive lanes) through the device hook -> uint32 array [len(rows) * lanes, out_words]"""
    inp = np.array([inw for _, inw in rows], dtype=np.uint32).reshape(len(rows), op.in_words)
    inp = np.ascontiguousarray(np.repeat(inp, lanes, axis=0))
    out = np.zeros((inp.shape[0], op.out_words), np.uint32)
    code = V.CODES[op.name] | (V.CHAIN if chain else 0)
    rc = lib.mi355zk_selftest_dev_op(code, which, inp.ctypes.data, op.in_words, out.ctypes.data, op.out_words, inp.shape[0])
    assert rc == 0, "mi355zk_selftest_dev_op(%s%s, %d) returned %d" % (op.name, "|CHAIN" if chain else "", which, rc)
    return out


def check_all(op, which, rows, outs, verify=None):
    """verify every row; report the first failures by op, field, class and operands"""
    bad = []
    for (cls, inw), outw in zip(rows, outs):
        try:
            (verify or op.verify)(which, inw, outw, op.expect(which, inw))
        except AssertionError as e:
            bad.append("%s: %s" % (op.describe(which, cls, inw), e))
    assert not bad, "%d of %d cases wrong, first:\n%s" % (len(bad), len(rows), "\n".join(bad[:5]))


def same(op, which, rows, a, b, what):
    diff = np.nonzero((a != b).any(axis=1))[0]
    assert diff.size == 0, "%s differ in %d cases, first: %s\n  %s\n  %s" % (what, diff.size, op.describe(which, *rows[diff[0]]), V.hexw(a[diff[0]]),
                                                                             V.hexw(b[diff[0]]))


@pytest.mark.parametrize("name,which", [(op.name, w) for op in V.FP_OPS + V.FQ2_OPS + V.F2U_OPS for w in op.fields])
def test_field_ops(lib, name, which):
    op = V.BY_NAME[name]
    rows = op.table(which)
    check_all(op, which, rows, run(lib, op, which, rows))


@pytest.mark.parametrize("name,which", [(op.name, w) for op in V.U_OPS for w in op.fields])
def test_uform_ops(lib, name, which):
    op = V.BY_NAME[name]
    rows = op.table(which)
    plain = run(lib, op, which, rows)
    check_all(op, which, rows, plain)
    same(op, which, rows, plain, run(lib, op, which, rows, chain=True), "the plain and the ZK_CHAIN_MAD build")
    if op.host:
        host = np.array([_host_call(lib, op, which, inw) for _, inw in rows], dtype=np.uint32)
        same(op, which, rows, plain, host, "the device and the host-compiled hook")


ONE_LANE = [op for op in V.GROUP_OPS + V.JAC_OPS if op.group == 1]


@pytest.mark.parametrize("name", [op.name for op in ONE_LANE])
def test_group_law_one_lane(lib, name):
    op = V.BY_NAME[name]
    rows = op.table(0)
    plain = run(lib, op, 0, rows)
    check_all(op, 0, rows, plain)
    if op.chain:
        same(op, 0, rows, plain, run(lib, op, 0, rows, chain=True), "the plain and the ZK_CHAIN_MAD build")


# (the Fq2 code is never built with ZK_CHAIN_MAD: no G2 / chain combination is shipped)
@pytest.mark.parametrize("g,chain", [("G1", False), ("G1", True), ("G2", False)])
def test_quad_addition_every_lane(lib, g, chain):
    """xyzzr_add_quad: four lanes per addition, the case replicated over the quad as the kernels hold it; EVERY lane's result is the model's
    sum and the same limbs, and its record is byte-identical to the one-lane xyzzr_add's"""
    op, one = V.BY_NAME[g + "_RADD_QUAD"], V.BY_NAME[g + "_RADD"]
    assert op.chain or not chain
    rows = op.table(0)
    assert [r[1] for r in rows] == [r[1] for r in one.table(0)[:len(rows) - V.N_RANDOM_GROUPS]] + [r[1] for r in rows[-V.N_RANDOM_GROUPS:]]
    out = run(lib, op, 0, rows, chain=chain, lanes=4).reshape(len(rows), 4, op.out_words)
    ref = run(lib, one, 0, rows, chain=chain)
    A = 4 * op.g.uw
    for lane in range(4):
        check_all(op, 0, rows, out[:, lane])
        same(op, 0, rows, out[:, lane, A:], ref[:, A:], "the record of lane %d of the quad and of the one-lane addition" % lane)
        same(op, 0, rows, out[:, lane], out[:, 0], "lane %d and lane 0 of the quad" % lane)


@pytest.mark.parametrize("g,chain", [("G1", False), ("G1", True), ("G2", False)])
def test_pair_addition_both_lanes(lib, g, chain):
    """pair_add_mixed: the even lane holds (X, ZZ), the odd lane (Y, ZZZ); together they are the model's sum, and the record they write is
    byte-identical to the one-lane xyzzu_add_mixed's"""
    op, one = V.BY_NAME[g + "_PAIR_ADD_MIXED"], V.BY_NAME[g + "_ADD_MIXED"]
    assert op.chain or not chain
    rows = op.table(0)
    out = run(lib, op, 0, rows, chain=chain, lanes=2).reshape(len(rows), 2, op.out_words)
    ref = run(lib, one, 0, rows, chain=chain)
    A = 4 * op.g.uw
    bad = []
    for i, (cls, inw) in enumerate(rows):
        try:
            rec = op.verify_pair(inw, out[i, 0], out[i, 1], op.expect(0, inw))
            assert rec == [int(x) for x in ref[i, A:]], "record %s, the one-lane addition writes %s" % (V.hexw(rec), V.hexw(ref[i, A:]))
        except AssertionError as e:
            bad.append("%s: %s" % (op.describe(0, cls, inw), e))
    assert not bad, "%d of %d cases wrong, first:\n%s" % (len(bad), len(rows), "\n".join(bad[:5]))


@pytest.mark.parametrize("gname,what", [(g, w) for g in ("G1", "G2") for w in ("ADD_MIXED", "PAIR_ADD_MIXED", "RADD", "RADD_QUAD")])
def test_chains_feed_device_results_back(lib, gname, what):
    """field_edge_vectors.chain_schedule: 64 signed additions into one accumulator with an infinity, a repeat and a negation planted, N_CHAINS
    chains side by side (neighbouring lanes / groups hold different chains).  The accumulator of step k + 1 is the limb vector the DEVICE
    returned at step k, so the lazily reduced values are the ones the kernels reach; every step is checked against bn254_model and the
    invariant X < 6p, Y, ZZ, ZZZ < 2p (dec_point), in every lane of a quad / pair."""
    op = V.BY_NAME["%s_%s" % (gname, what)]
    g, A = op.g, 4 * op.g.uw
    mixed = "MIXED" in what
    scheds = [V.chain_schedule(g, c) for c in range(V.N_CHAINS)]
    accs = [[0] * A for _ in scheds]
    rnd = V._rng("chain-operands" + op.name, 0)
    for step in range(V.CHAIN_STEPS):
        rows = []
        for c, sched in enumerate(scheds):
            pt, neg, _ = sched[step]
            if mixed:
                second = g.coord_words(pt[0]) + g.coord_words(pt[1]) + [int(neg)]
            else:
                second = V.enc_point(g, g.neg(pt) if neg else pt, V._rand_z(g, rnd), V._lift_sets(g, rnd)[2][1], 261)
            rows.append(("chain %d step %d (%s)" % (c, step, V.CHAIN_PLANTS.get(step, "random base")), accs[c] + second))
        out = run(lib, op, 0, rows, lanes=op.group).reshape(len(rows), op.group, op.out_words)
        for c, (cls, inw) in enumerate(rows):
            want = scheds[c][step][2]
            try:
                if op.group == 2:
                    e, o = [int(x) for x in out[c, 0]], [int(x) for x in out[c, 1]]
                    uw = g.uw
                    accs[c] = e[:uw] + o[:uw] + e[uw:2 * uw] + o[uw:2 * uw]
                    op.verify_pair(inw, e, o, {"pt": want})
                else:
                    for lane in range(op.group):
                        op.verify(0, inw, out[c, lane], {"pt": want})
                        assert (out[c, lane] == out[c, 0]).all(), "lane %d and lane 0 differ" % lane
                    accs[c] = [int(x) for x in out[c, 0, :A]]
            except AssertionError as e:
                raise AssertionError("%s: %s" % (op.describe(0, cls, inw), e)) from None


def _dev_fr(zk, lib, fn, a, b=None):
    """a public elementwise Fr entry point on device buffers: a (and b) are [n, 8] uint32 -> the result"""
    import ctypes as C

    n = a.shape[0]
    bufs = []
    for arr in (a, b):
        if arr is None:
            bufs.append(None)
            continue
        p = C.c_void_p()
        assert lib.mi355zk_malloc(C.byref(p), arr.nbytes) == 0
        assert lib.mi355zk_memcpy_h2d(p, arr.ctypes.data, arr.nbytes) == 0
        bufs.append(p)
    try:
        if b is None:
            assert fn(bufs[0], bufs[0], n, None) == 0
        else:
            assert fn(bufs[0], bufs[1], n, None) == 0
        assert lib.mi355zk_sync(None) == 0
        out = np.zeros_like(a)
        assert lib.mi355zk_memcpy_d2h(out.ctypes.data, bufs[0], a.nbytes) == 0
        return out
    finally:
        for p in bufs:
            if p is not None:
                lib.mi355zk_free(p)


def test_public_fr_entry_points_over_the_table(zk, lib):
    """mi355zk_bn254_fr_mul_assign_dev / _sub_assign_dev / _into_repr_dev take caller field data and need no hook: the Fr rows of the table
    against big ints.  Canonical operands only: include/mi355zk.h declares the result for an element >= r UNDEFINED (the kernels do not check,
    the call returns 0), so there is nothing to assert for such rows beyond what the header says -- and a test below pins that sentence."""
    r = M.R_ORDER
    ri = pow(1 << 256, -1, r)
    for name, fn, ref in (("FP_MUL", lib.mi355zk_bn254_fr_mul_assign_dev, lambda a, b: a * b * ri % r),
                          ("FP_SUB", lib.mi355zk_bn254_fr_sub_assign_dev, lambda a, b: (a - b) % r)):
        op = V.BY_NAME[name]
        rows = op.table(1)
        arr = np.array([inw for _, inw in rows], dtype=np.uint32)
        out = _dev_fr(zk, lib, fn, np.ascontiguousarray(arr[:, :8]), np.ascontiguousarray(arr[:, 8:]))
        for (cls, inw), o in zip(rows, out):
            assert V.v32(o) == ref(V.v32(inw[:8]), V.v32(inw[8:])), op.describe(1, cls, inw)
    op = V.BY_NAME["FP_SQR"]
    rows = op.table(1)
    arr = np.ascontiguousarray(np.array([inw for _, inw in rows], dtype=np.uint32))
    out = _dev_fr(zk, lib, lib.mi355zk_bn254_fr_into_repr_dev, arr)
    for (cls, inw), o in zip(rows, out):
        assert V.v32(o) == V.v32(inw) * ri % r, op.describe(1, cls, inw)


def test_header_states_the_operand_range_of_the_fr_entry_points():
    import os

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mi355zk.h")).read()
    block = text[text.index("elementwise Fr operations"):text.index("mi355zk_bn254_fr_into_repr_dev(")]
    assert "CANONICAL value < r" in block and "UNDEFINED" in block
