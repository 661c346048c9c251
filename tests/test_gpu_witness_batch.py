"""Witness batches on the device (csrc/r1cs.hip): mi355zk_bn254_fr_sparse_matvec_batch_dev against the single-vector call and Python big
ints, mi355zk_bn254_fr_r1cs_check_dev against mi355zk_selftest_r1cs_check (the same predicate on the host) and planted failures, and
circom.prepare_provers_dev / first_unsatisfied / prove(check=) against prepare_prover_dev, prepare_prover and prove."""
import ctypes as C

import numpy as np
import pytest

import bn254_model as M
import inputs
import oracle_lib as O
import r1cs_cases as K
import witness_cases as W

pytestmark = pytest.mark.gpu

r = K.R_ORDER
SENTINEL = 0x5A5A5A5A5A5A5A5A
V = 1                      # lib.R1CS_BATCH_V, the tile of the batch kernel (asserted below)
N_VECTORS = sorted({1, 2, V - 1, V, V + 1, 2 * V + 1} - {0})   # (0 vectors: refused, tests/test_witness_check_host.py)


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _ptr(t, element=0):
    return C.c_void_p(t.data_ptr() + 32 * element) if t is not None and t.numel() else None


def _stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- the batch product
# The row-length mix of tests/test_gpu_r1cs.py (every length 0 .. 130 twice, 191 .. 193, 255 .. 257, 1000, 4097, the (r - 1)(r - 1) row, 300
# rows of 0 .. 5 terms, shuffled over three workgroups) times 2 V + 1 vectors: the big-int rows and the single-vector call's rows, once.
@pytest.fixture(scope="module")
def matrix(zk, worker):
    import torch

    rng = np.random.default_rng(5400)
    n_x, n_coeffs, n_vec = 500, 40, max(N_VECTORS)

    def uniform(k):
        return [int.from_bytes(rng.bytes(40), "little") % r for _ in range(k)]

    xs = [uniform(n_x) for _ in range(n_vec)]
    for v, x in enumerate(xs):
        x[0], x[1], x[2], x[499] = 0, 1, r - 1, (r - 1 - v) % r
    coeffs = uniform(n_coeffs)
    coeffs[0], coeffs[1], coeffs[2], coeffs[39] = 1, r - 1, 0, 2
    lengths = list(range(131)) * 2 + [191, 192, 193, 255, 256, 257, 1000, 4097] + [-1] + [int(v) for v in rng.integers(0, 6, size=300)]
    rows = []
    for i in rng.permutation(len(lengths)):
        ln = lengths[i]
        if ln < 0:
            rows.append([(2, 1)] * 100)                                    # (col 2, coeff 1): r - 1 times r - 1, a hundred times
        else:
            rows.append([(int(v), int(c)) for v, c in zip(rng.integers(0, n_x, size=ln), rng.integers(0, n_coeffs, size=ln))])
    row_ptr = np.concatenate([[0], np.cumsum([len(t) for t in rows])]).astype(np.uint32)
    mx = {"n_x": n_x, "n_coeffs": n_coeffs, "n_rows": len(rows), "nnz": int(row_ptr[-1]), "lengths": [len(t) for t in rows],
          "x": [K.mont(x) for x in xs], "want": [K.mont(sum(coeffs[c] * x[v] for v, c in t) for t in rows) for x in xs]}
    mx["d"] = {"row_ptr": _dev(row_ptr), "col": _dev(np.array([v for t in rows for v, _ in t], dtype=np.uint32)),
               "cid": _dev(np.array([c for t in rows for _, c in t], dtype=np.uint32)), "coeffs": _dev(K.mont(coeffs))}
    d, single = mx["d"], []
    for x in mx["x"]:                                                      # what the single-vector call writes for every vector
        out, dx = torch.zeros((len(rows), 4), dtype=torch.int64, device="cuda"), _dev(x)
        assert zk.lib.load().mi355zk_bn254_fr_sparse_matvec_dev(_ptr(out), _ptr(d["row_ptr"]), _ptr(d["col"]), _ptr(d["cid"]), _ptr(d["coeffs"]),
                                                                n_coeffs, _ptr(dx), n_x, len(rows), mx["nnz"], _stream()) == 0
        single.append(_host(out))
    mx["single"] = single
    return mx


@pytest.mark.parametrize("n_vectors", N_VECTORS)
def test_batch_product_equals_the_single_call_and_big_ints(zk, worker, matrix, n_vectors):
    import torch

    mx, d = matrix, matrix["d"]
    assert V == zk.lib.R1CS_BATCH_V
    assert mx["n_rows"] > 2 * 256 and {0, 16, 17, 63, 64, 65, 128, 129, 4097} <= set(mx["lengths"])
    n_x, x_stride = mx["n_x"], mx["n_x"] + 3
    x_host = np.full((n_vectors * x_stride + 3, 4), SENTINEL, dtype=np.uint64)     # a sentinel in every gap and after the last vector
    for v in range(n_vectors):
        x_host[v * x_stride:v * x_stride + n_x] = mx["x"][v]
    dx = _dev(x_host)
    for n_rows in (mx["n_rows"], 1, 255, 256, 257):
        out_stride = n_rows + 5
        out = torch.full((n_vectors * out_stride + 5, 4), SENTINEL, dtype=torch.int64, device="cuda")
        rc = zk.lib.load().mi355zk_bn254_fr_sparse_matvec_batch_dev(_ptr(out), out_stride, _ptr(d["row_ptr"]), _ptr(d["col"]), _ptr(d["cid"]),
                                                                    _ptr(d["coeffs"]), mx["n_coeffs"], _ptr(dx), n_x, x_stride, n_vectors, n_rows,
                                                                    mx["nnz"], _stream())
        assert rc == 0
        got = _host(out)
        for v in range(n_vectors):
            rows = got[v * out_stride:v * out_stride + n_rows]
            bad = np.nonzero((rows != mx["want"][v][:n_rows]).any(axis=1))[0]
            assert bad.size == 0, (n_rows, v, [(int(i), mx["lengths"][i]) for i in bad[:8]])
            assert rows.tobytes() == mx["single"][v][:n_rows].tobytes(), (n_rows, v)   # the single call's bytes
            assert rows.tobytes() == mx["want"][v][:n_rows].tobytes(), (n_rows, v)     # the big-int model's
            assert (got[v * out_stride + n_rows:(v + 1) * out_stride] == SENTINEL).all(), (n_rows, v)   # the gap after vector v
        assert (got[n_vectors * out_stride:] == SENTINEL).all(), n_rows
    assert _host(dx).tobytes() == x_host.tobytes()                         # x and its gaps are as they were


# ---- the satisfaction check
def _selftest(zk, a, b, c):
    first, count = C.c_longlong(99), C.c_uint32(99)
    p = lambda x: np.ascontiguousarray(x).ctypes.data_as(C.c_void_p)  # noqa: E731
    assert zk.lib.load().mi355zk_selftest_r1cs_check(p(a), p(b), p(c), a.shape[0], C.byref(first), C.byref(count)) == 0
    return first.value, count.value


@pytest.mark.parametrize("n_rows", [1, 63, 64, 65, 255, 256, 257, 1000])
def test_r1cs_check_finds_the_planted_rows(zk, worker, n_rows):
    """Three vectors of n_rows rows, vector_stride > n_rows with failing rows (1 * 1 = 2) in every gap; failures planted as c + 1.  Every
    verdict against the plan, and against mi355zk_selftest_r1cs_check on the same bytes."""
    n_vec, gap = 3, 7
    chk = zk.lib.load().mi355zk_bn254_fr_r1cs_check_dev
    rng = np.random.default_rng(5500 + n_rows)
    uni = lambda: int.from_bytes(rng.bytes(40), "little") % r  # noqa: E731
    a = [[uni() for _ in range(n_rows)] for _ in range(n_vec)]
    b = [[uni() for _ in range(n_rows)] for _ in range(n_vec)]
    for v in range(n_vec):
        a[v][0], b[v][n_rows // 2] = 0, 0                                  # 0 x = 0 and x 0 = 0 among the rows
    ma, mb = [K.mont(x) for x in a], [K.mont(x) for x in b]
    one, two = K.mont([1])[0], K.mont([2])[0]
    single = [{1: [row]} for row in sorted({0, 63, 64, 255, 256, n_rows - 1}) if row < n_rows]
    several = sorted({n_rows - 1, n_rows // 2, n_rows // 3, min(64, n_rows - 1), min(3, n_rows - 1)})
    plans = [{}] + single + [{2: several}, {0: [n_rows - 1], 1: [0], 2: [n_rows // 2]}, {0: several, 1: [n_rows - 1], 2: several[1:] or [0]}]
    for plan in plans:
        mc = []
        for v in range(n_vec):
            c = [x * y % r for x, y in zip(a[v], b[v])]
            for row in plan.get(v, []):
                c[row] = (c[row] + 1) % r
            mc.append(K.mont(c))
        want = [(plan[v][0], len(plan[v])) if plan.get(v) else (-1, 0) for v in range(n_vec)]
        assert [_selftest(zk, ma[v], mb[v], mc[v]) for v in range(n_vec)] == want, plan    # the host run of the predicate, same bytes
        for layout in ("one array", "three arrays"):
            if layout == "one array":                                      # a = buf, b = buf + (n_rows + gap), c = buf + 2 (n_rows + gap)
                part, stride = n_rows + gap, 3 * (n_rows + gap)
                buf = np.empty((n_vec * stride, 4), dtype=np.uint64)
                buf[:] = two
                for v in range(n_vec):
                    for k, src in enumerate((ma[v], mb[v], mc[v])):
                        buf[v * stride + k * part:v * stride + k * part + n_rows] = src
                        if k < 2:
                            buf[v * stride + k * part + n_rows:v * stride + (k + 1) * part] = one
                t = _dev(buf)
                ptrs = (_ptr(t), _ptr(t, part), _ptr(t, 2 * part))
            else:
                stride = n_rows + gap
                arrays = []
                for k, src in enumerate((ma, mb, mc)):
                    buf = np.empty((n_vec * stride, 4), dtype=np.uint64)
                    buf[:] = one if k < 2 else two
                    for v in range(n_vec):
                        buf[v * stride:v * stride + n_rows] = src[v]
                    arrays.append(_dev(buf))
                ptrs = tuple(_ptr(t) for t in arrays)
            first, count = (C.c_longlong * n_vec)(*[99] * n_vec), (C.c_uint32 * n_vec)(*[99] * n_vec)
            assert chk(*ptrs, n_rows, stride, n_vec, first, count, _stream()) == 0
            assert list(zip(first, count)) == want, (plan, layout)
            first = (C.c_longlong * n_vec)(*[99] * n_vec)
            assert chk(*ptrs, n_rows, stride, n_vec, first, None, _stream()) == 0 and list(first) == [w[0] for w in want]   # n_bad may be NULL


# ---- circom.prepare_provers_dev / first_unsatisfied / prove(check=)
@pytest.fixture(scope="module")
def satisfied(zk):
    return W.satisfied_circuit(zk)


def _same_assignment(got, ref, m, what):
    for name in ("a", "b", "c"):
        g = getattr(got, name)
        assert g.shape == (m, 4) and g.is_contiguous() and _host(g).tobytes() == _host(getattr(ref, name)).tobytes(), (what, name)
    for name in ("input_assignment", "aux_assignment"):
        assert _host(getattr(got, name)).tobytes() == _host(getattr(ref, name)).tobytes(), (what, name)
    for name in ("a_aux_density", "b_input_density", "b_aux_density"):
        (gw, gn), (ww, wn) = getattr(got, name).words(), getattr(ref, name).words()
        assert gn == wn and np.array_equal(gw, ww) and getattr(got, name).get_total_density() == getattr(ref, name).get_total_density()


@pytest.mark.parametrize("which", ["small", "satisfied"])
def test_prepare_provers_dev_matches_prepare_prover_dev(zk, worker, satisfied, which):
    import torch

    dev = torch.device("cuda", 0)
    if which == "small":
        circuit = K.small_circuit(zk)
        ws = [list(circuit.witness) for _ in range(5)]
        for k in range(1, 5):
            ws[k][2 + k] = (ws[k][2 + k] + 1000 * k) % r                   # (any values: nothing here asks for a satisfied witness)
    else:
        circuit = satisfied.circuit
        ws = [circuit.witness] + [satisfied.witness() for _ in range(4)]
    cc = zk.circom.compile_circuit(circuit, dev)
    for n_batch in (1, 5):
        refs = [zk.circom.prepare_prover_dev(cc, w) for w in ws[:n_batch]]
        frozen = np.stack([K.to_limbs(w) for w in ws[:n_batch]])
        frozen.flags.writeable = False
        forms = {"lists": ws[:n_batch], "arrays": [K.to_limbs(w) for w in ws[:n_batch]], "one array": np.stack([K.to_limbs(w) for w in ws[:n_batch]]),
                 "read-only array": frozen}
        for form, witnesses in forms.items():
            got = zk.circom.prepare_provers_dev(cc, witnesses)
            assert len(got) == n_batch
            for v in range(n_batch):
                _same_assignment(got[v], refs[v], cc.m, (which, n_batch, form, v))
                assert got[v].a.untyped_storage().data_ptr() == got[0].a.untyped_storage().data_ptr()       # views of ONE product
                assert got[v].aux_assignment.untyped_storage().data_ptr() == got[0].input_assignment.untyped_storage().data_ptr()
            if which == "satisfied":
                assert zk.circom.first_unsatisfied(got) == [(None, 0)] * n_batch
                assert len(zk.circom.prepare_provers_dev(cc, witnesses, check=True)) == n_batch
    if which == "small":
        assert zk.circom.first_unsatisfied(zk.circom.prepare_provers_dev(cc, [ws[0]])) == [(None, 0)]      # 2 * 3 = 6, (6 + 5) * 1 = 11, (...) * 0 = 0


def test_first_unsatisfied_names_the_witness_and_the_constraint(zk, worker, satisfied):
    import torch

    s, circuit = satisfied, satisfied.circuit
    dev = torch.device("cuda", 0)
    cc = zk.circom.compile_circuit(circuit, dev)
    ws = [s.witness() for _ in range(5)]
    ws[2] = s.break_witness(ws[2], [17])
    ws[4] = s.break_witness(ws[4], [3, 250])
    want = [(None, 0), (None, 0), (17, 1), (None, 0), (3, 2)]
    provers = zk.circom.prepare_provers_dev(cc, ws)
    assert zk.circom.first_unsatisfied(provers) == want                    # one call over the batch
    assert zk.circom.first_unsatisfied(provers[4]) == [(3, 2)]             # one assignment
    assert zk.circom.first_unsatisfied([provers[3], provers[2], provers[4]]) == [(None, 0), (17, 1), (3, 2)]   # not equally spaced: one call each
    assert zk.circom.first_unsatisfied([zk.circom.prepare_prover_dev(cc, w) for w in ws]) == want              # separate allocations
    with pytest.raises(zk.circom.UnsatisfiedConstraint) as e:
        zk.circom.prepare_provers_dev(cc, ws, check=True)
    err = e.value
    assert isinstance(err, zk.SynthesisError) and err.kind == "Unsatisfiable"
    assert (err.witness, err.index, err.count) == (2, 17, 1)
    assert (err.a, err.b, err.c) == W.row_values(circuit, ws[2], 17) and err.a * err.b % r != err.c
    with pytest.raises(zk.circom.UnsatisfiedConstraint) as e:
        zk.circom.prepare_provers_dev(cc, [ws[0], ws[4]], check=True)
    assert (e.value.witness, e.value.index, e.value.count) == (1, 3, 2)
    assert (e.value.a, e.value.b, e.value.c) == W.row_values(circuit, ws[4], 3)
    # an assignment of the Python prepare_prover: n rows (no padding), three tensors of their own
    assert zk.circom.first_unsatisfied(zk.circom.prepare_prover(circuit, dev)) == [(None, 0)]
    broken = s.break_coefficient(zk, [17, 299])
    assert zk.circom.first_unsatisfied(zk.circom.prepare_prover(broken, dev)) == [(17, 2)]
    mixed = [zk.circom.prepare_prover(broken, dev), zk.circom.prepare_prover_dev(cc, ws[1]), provers[2]]
    assert zk.circom.first_unsatisfied(mixed) == [(17, 2), (None, 0), (17, 1)]


def test_prove_with_check(zk, worker):
    """prove(..., compiled=cc, check=True): the proof of prove(..., compiled=cc) on a satisfied witness, UnsatisfiedConstraint on a broken
    one; prove_many likewise.  Parameters made the way tests/test_gpu_r1cs.py makes them, for a satisfied circuit of 60 constraints."""
    import torch

    s = W.satisfied_circuit(zk, seed=5300, n_constraints=60, num_inputs=3, num_aux=12)
    circuit = s.circuit
    cs = zk.circom.assemble(circuit)
    power = zk.circom.domain_exponent(cs.num_constraints)
    m = 1 << power
    tau, alpha, beta = 0x1234567 % r, 0x89ABCDEF01 % r, 0x55AA55AA55 % r
    limbs = lambda ks: np.stack([np.array(M.to_limbs(k % r), dtype=np.uint64) for k in ks])  # noqa: E731
    mul1 = lambda ks: O.G1.mul_many_affine(inputs.G1_GEN_RAW, limbs(ks))  # noqa: E731
    mul2 = lambda ks: O.G2.mul_many_affine(inputs.G2_GEN_RAW, limbs(ks))  # noqa: E731
    tp = [pow(tau, i, r) for i in range(2 * m - 1)]
    acc = {"hash": torch.zeros(64, dtype=torch.uint8).cuda(), "tau_g1": _dev(mul1(tp)), "tau_g2": _dev(mul2(tp[:m])),
           "alpha_g1": _dev(mul1([alpha * t for t in tp[:m]])), "beta_g1": _dev(mul1([beta * t for t in tp[:m]])), "beta_g2": _dev(mul2([beta]))}
    radix = zk.ceremony.read_phase1radix2m(zk.ceremony.write_phase1radix2m(zk.ceremony.prepare_phase2(acc, m)), m)
    params = zk.circom.mpc_parameters_new(circuit, False, radix)["params"]
    rr, ss = 0x1234567890ABCDEF1122334455667788 % r, 0x0FEDCBA9876543210F1E2D3C4B5A6978 % r
    cc = zk.circom.compile_circuit(circuit, params["h"].device)
    want = zk.circom.prove(worker, circuit, params, rr, ss, compiled=cc)
    got = zk.circom.prove(worker, circuit, params, rr, ss, compiled=cc, check=True)
    assert len(got) == 3 and all(np.array_equal(g, w) for g, w in zip(got, want)) and all(np.asarray(g).any() for g in got)
    plain = zk.circom.prove(worker, circuit, params, rr, ss, check=True)   # the Python prepare_prover, checked on the device
    assert all(np.array_equal(g, w) for g, w in zip(plain, want))
    bad = zk.circom.CircomCircuit(circuit.num_inputs, circuit.num_aux, circuit.num_constraints, circuit.constraints, s.break_witness(circuit.witness, [5]))
    for compiled in (cc, None):
        with pytest.raises(zk.circom.UnsatisfiedConstraint) as e:
            zk.circom.prove(worker, bad, params, rr, ss, compiled=compiled, check=True)
        assert (e.value.witness, e.value.index, e.value.count) == (0, 5, 1)
        assert (e.value.a, e.value.b, e.value.c) == W.row_values(bad, bad.witness, 5)
    w2 = s.witness()
    many = zk.circom.prove_many(worker, circuit, params, [circuit.witness, w2], [rr, ss], [ss, rr], compiled=cc, check=True)
    assert all(np.array_equal(g, w) for g, w in zip(many[0], want)) and len(many) == 2
    with pytest.raises(zk.circom.UnsatisfiedConstraint) as e:
        zk.circom.prove_many(worker, circuit, params, [circuit.witness, s.break_witness(w2, [59])], [rr, ss], [ss, rr], compiled=cc, check=True)
    assert (e.value.witness, e.value.index) == (1, 59)
