"""The R1CS evaluation on the device (csrc/r1cs.hip: mi355zk_bn254_fr_sparse_matvec[_check]_dev, mi355zk_bn254_fr_from_repr_dev) against
Python big ints, and circom.compile_circuit / prepare_prover_dev / prove(compiled=) against the existing circom.prepare_prover / prove."""
import ctypes as C

import numpy as np
import pytest

import bn254_model as M
import inputs
import oracle_lib as O
import r1cs_cases as K

pytestmark = pytest.mark.gpu

r = K.R_ORDER
SENTINEL = 0x5A5A5A5A5A5A5A5A


def _dev(a):
    import torch

    a = np.ascontiguousarray(a)
    view = {np.dtype(np.uint64): np.int64, np.dtype(np.uint32): np.int32}.get(a.dtype)
    return torch.from_numpy(a.view(view) if view else a).cuda()


def _host(t):
    return t.cpu().numpy().view(np.uint64)


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


# ---- the raw product
# Row lengths: every length 0 .. 130 twice (either side of a wave, of two waves and of the short-row threshold of r1cs.hip, 16, which
# lies inside 1 .. 129), 191 .. 193, 255 .. 257, 1000 and 4097 (either side of a workgroup and of several 64-lane strides), one row of
# (r - 1) * (r - 1) terms only, and 300 rows of 0 .. 5 terms; shuffled, so that long and short rows share the three workgroups.
@pytest.fixture(scope="module")
def matrix():
    rng = np.random.default_rng(4200)
    n_x, n_coeffs = 500, 40

    def uniform(k):
        return [int.from_bytes(rng.bytes(40), "little") % r for _ in range(k)]

    x = uniform(n_x)
    coeffs = uniform(n_coeffs)
    x[0], x[1], x[2], x[499] = 0, 1, r - 1, r - 1
    coeffs[0], coeffs[1], coeffs[2], coeffs[39] = 1, r - 1, 0, 2
    lengths = list(range(131)) * 2 + [191, 192, 193, 255, 256, 257, 1000, 4097] + [-1] + [int(v) for v in rng.integers(0, 6, size=300)]
    order = rng.permutation(len(lengths))
    rows = []
    for i in order:
        ln = lengths[i]
        if ln < 0:
            rows.append([(2, 1)] * 100)                                    # (col 2, coeff 1): r - 1 times r - 1, a hundred times
        else:
            rows.append([(int(v), int(c)) for v, c in zip(rng.integers(0, n_x, size=ln), rng.integers(0, n_coeffs, size=ln))])
    row_ptr = np.concatenate([[0], np.cumsum([len(t) for t in rows])]).astype(np.uint32)
    col = np.array([v for t in rows for v, _ in t], dtype=np.uint32)
    cid = np.array([c for t in rows for _, c in t], dtype=np.uint32)
    want = K.mont(sum(coeffs[c] * x[v] for v, c in t) for t in rows)      # the Montgomery form of the row's value: order-free, canonical
    return {"n_x": n_x, "n_coeffs": n_coeffs, "n_rows": len(rows), "nnz": int(row_ptr[-1]), "row_ptr": row_ptr, "col": col, "cid": cid,
            "x": K.mont(x), "coeffs": K.mont(coeffs), "want": want, "lengths": [len(t) for t in rows]}


def _matvec(zk, mx, n_rows, d=None):
    import torch

    d = d or {k: _dev(mx[k]) for k in ("row_ptr", "col", "cid", "x", "coeffs")}
    out = torch.full((mx["n_rows"] + 3, 4), SENTINEL, dtype=torch.int64, device="cuda")
    rc = zk.lib.load().mi355zk_bn254_fr_sparse_matvec_dev(_ptr(out), _ptr(d["row_ptr"]), _ptr(d["col"]), _ptr(d["cid"]), _ptr(d["coeffs"]),
                                                          mx["n_coeffs"], _ptr(d["x"]), mx["n_x"], n_rows, mx["nnz"], _stream())
    assert rc == 0
    return _host(out)


def test_sparse_matvec_every_row_length_against_big_ints(zk, worker, matrix):
    mx = matrix
    assert mx["n_rows"] > 2 * 256 and {0, 16, 17, 63, 64, 65, 128, 129, 4097} <= set(mx["lengths"])
    d = {k: _dev(mx[k]) for k in ("row_ptr", "col", "cid", "x", "coeffs")}
    assert zk.lib.load().mi355zk_bn254_fr_sparse_matvec_check_dev(_ptr(d["row_ptr"]), _ptr(d["col"]), _ptr(d["cid"]), mx["n_coeffs"], mx["n_x"],
                                                                  mx["n_rows"], mx["nnz"], _stream()) == 0
    for n_rows in (mx["n_rows"], 1, 255, 256, 257):
        got = _matvec(zk, mx, n_rows, d)
        bad = np.nonzero((got[:n_rows] != mx["want"][:n_rows]).any(axis=1))[0]
        assert bad.size == 0, (n_rows, [(int(i), mx["lengths"][i]) for i in bad[:8]])
        assert got[:n_rows].tobytes() == mx["want"][:n_rows].tobytes()
        assert (got[n_rows:] == SENTINEL).all(), n_rows                    # nothing written past the rows asked for


def test_sparse_matvec_without_terms_writes_zeros(zk, worker):
    import torch

    n_rows = 300
    row_ptr = torch.zeros(n_rows + 1, dtype=torch.int32, device="cuda")
    x = _dev(K.mont([5, 6]))
    out = torch.full((n_rows + 1, 4), SENTINEL, dtype=torch.int64, device="cuda")
    rc = zk.lib.load().mi355zk_bn254_fr_sparse_matvec_dev(_ptr(out), _ptr(row_ptr), None, None, None, 0, _ptr(x), 2, n_rows, 0, _stream())
    assert rc == 0
    got = _host(out)
    assert not got[:n_rows].any() and (got[n_rows:] == SENTINEL).all()
    assert zk.lib.load().mi355zk_bn254_fr_sparse_matvec_check_dev(_ptr(row_ptr), None, None, 0, 2, n_rows, 0, _stream()) == 0


def test_check_call_reports_an_invalid_structure(zk, worker, matrix):
    """Only the CHECKING call sees the invalid matrices: the evaluating call is never run on them."""
    mx = matrix
    chk = zk.lib.load().mi355zk_bn254_fr_sparse_matvec_check_dev

    def check(row_ptr=mx["row_ptr"], col=mx["col"], cid=mx["cid"], n_rows=mx["n_rows"], nnz=mx["nnz"]):
        d = [_dev(a) for a in (row_ptr, col, cid)]
        return chk(_ptr(d[0]), _ptr(d[1]), _ptr(d[2]), mx["n_coeffs"], mx["n_x"], n_rows, nnz, _stream())

    assert check() == 0
    t = mx["nnz"] - 7
    col = mx["col"].copy()
    col[t] = mx["n_x"]
    assert check(col=col) == 3                                             # one col out of range
    cid = mx["cid"].copy()
    cid[12345] = mx["n_coeffs"] + 1000
    assert check(cid=cid) == 3                                             # one coeff_id out of range
    rp = mx["row_ptr"].copy()
    k = int(np.argmax(np.diff(rp.astype(np.int64)) > 3))
    rp[k + 1] = rp[k] - 1 if rp[k] else rp[k + 2] + 1
    assert check(row_ptr=rp) == 3                                          # a decreasing row_ptr
    rp = mx["row_ptr"].copy()
    rp[0] = 1
    assert check(row_ptr=rp) == 3                                          # does not start at 0
    assert check(nnz=mx["nnz"] - 1) == 3                                   # does not end at nnz
    assert check() == 0


def test_from_repr_against_big_ints_and_into_repr(zk, worker):
    lib = zk.lib.load()
    rng = np.random.default_rng(4300)
    vals = [0, 1, r - 1] + [int.from_bytes(rng.bytes(40), "little") % r for _ in range(1000)]
    canon, want = K.to_limbs(vals), K.mont(vals)
    src = _dev(canon)
    dst = src.clone().zero_()
    assert lib.mi355zk_bn254_fr_from_repr_dev(_ptr(dst), _ptr(src), len(vals), _stream()) == 0        # out of place
    assert _host(dst).tobytes() == want.tobytes() and _host(src).tobytes() == canon.tobytes()
    assert lib.mi355zk_bn254_fr_from_repr_dev(_ptr(src), _ptr(src), len(vals), _stream()) == 0        # in place
    assert _host(src).tobytes() == want.tobytes()
    assert lib.mi355zk_bn254_fr_into_repr_dev(_ptr(src), _ptr(src), len(vals), _stream()) == 0        # into_repr o from_repr = identity
    assert _host(src).tobytes() == canon.tobytes()


@pytest.mark.parametrize("which", ["small", "random"])
def test_prepare_prover_dev_matches_prepare_prover(zk, worker, which):
    import torch

    circuit = K.small_circuit(zk) if which == "small" else K.random_circuit(zk)
    dev = torch.device("cuda", 0)
    ref = zk.circom.prepare_prover(circuit, dev)
    cc = zk.circom.compile_circuit(circuit, dev)
    n = len(circuit.constraints) + circuit.num_inputs
    m = 1 << zk.circom.domain_exponent(n)
    assert (cc.n, cc.m) == (n, m) and ref.a.shape[0] == n
    frozen = K.to_limbs(circuit.witness)
    frozen.flags.writeable = False
    forms = {"ints": list(circuit.witness), "array": K.to_limbs(circuit.witness), "read-only array": frozen}
    for form, witness in forms.items():
        got = zk.circom.prepare_prover_dev(cc, witness)
        for name in ("a", "b", "c"):
            g, w = _host(getattr(got, name)), _host(getattr(ref, name))
            assert g.shape == (m, 4) and g[:n].tobytes() == w.tobytes(), (form, name)
            assert not g[n:].any(), (form, name)                           # the padding rows wrote their zeros
            assert getattr(got, name).is_contiguous()
        for name in ("input_assignment", "aux_assignment"):
            assert _host(getattr(got, name)).tobytes() == _host(getattr(ref, name)).tobytes(), (form, name)
        for name in ("a_aux_density", "b_input_density", "b_aux_density"):
            (gw, gn), (ww, wn) = getattr(got, name).words(), getattr(ref, name).words()
            assert gn == wn and np.array_equal(gw, ww) and getattr(got, name).get_total_density() == getattr(ref, name).get_total_density()
    # the evaluation vectors go into the H pipeline as they are
    dom = zk.EvaluationDomain.from_coeffs(got.a)
    assert dom.exp == cc.exp and dom.coeffs.shape[0] == m


def test_prove_with_a_compiled_circuit_gives_the_same_proof(zk, worker):
    """prove(..., compiled=) against prove(...) on the ~200-constraint circuit, with parameters made the way
    tests/test_gpu_ceremony.py makes them: a radix file from an accumulator with known tau, alpha, beta."""
    import torch

    circuit = K.random_circuit(zk)
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
    want = zk.circom.prove(worker, circuit, params, rr, ss)
    cc = zk.circom.compile_circuit(circuit, params["h"].device)
    got = zk.circom.prove(worker, circuit, params, rr, ss, compiled=cc)
    assert len(got) == 3 and all(np.array_equal(g, w) for g, w in zip(got, want))
    assert all(np.asarray(g).any() for g in got)
    other = zk.circom.compile_circuit(K.small_circuit(zk), params["h"].device)
    with pytest.raises(ValueError):                                        # a compiled circuit of another circuit is refused
        zk.circom.prove(worker, circuit, params, rr, ss, compiled=other)
