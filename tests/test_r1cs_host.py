"""The R1CS evaluation's host side (no GPU): the three new ABI symbols, their argument rules, and the witness-independent half of
circom.compile_circuit (the CSR matrix and the density maps) against circom.prepare_prover."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import r1cs_cases as K

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("mi355zk_bn254_fr_sparse_matvec_dev", "mi355zk_bn254_fr_sparse_matvec_check_dev", "mi355zk_bn254_fr_from_repr_dev")


def _zk():
    import phase2_bn254_amd as zk

    return zk


def test_the_three_symbols_are_declared_exported_and_bound():
    zk = _zk()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mi355zk.h")).read(), flags=re.S)
    lib = zk.lib.load()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in zk.lib.SIGNATURES and hasattr(lib, name), name
    assert lib.mi355zk_abi_version() == 7


def test_bad_arguments_are_rejected_without_a_device():
    zk = _zk()
    lib = zk.lib.load()
    BAD = zk.lib.ERR_BAD_ARGS
    # host memory stands in for the device arrays: every call below is refused (or has nothing to do) before any device work
    buf = [np.zeros(64, np.uint64) for _ in range(6)]
    out, rp, col, cid, cf, x = (b.ctypes.data_as(C.c_void_p) for b in buf)
    mv, chk = lib.mi355zk_bn254_fr_sparse_matvec_dev, lib.mi355zk_bn254_fr_sparse_matvec_check_dev
    good = dict(out=out, rp=rp, col=col, cid=cid, cf=cf, n_coeffs=2, x=x, n_x=3, n_rows=4, nnz=5)

    def call(**kw):
        a = dict(good, **kw)
        return mv(a["out"], a["rp"], a["col"], a["cid"], a["cf"], a["n_coeffs"], a["x"], a["n_x"], a["n_rows"], a["nnz"], None)

    def check(**kw):
        a = dict(good, **kw)
        return chk(a["rp"], a["col"], a["cid"], a["n_coeffs"], a["n_x"], a["n_rows"], a["nnz"], None)

    for name in ("out", "rp", "col", "cid", "cf", "x"):                    # a NULL pointer with a non-zero count
        assert call(**{name: None}) == BAD, name
    for name in ("rp", "col", "cid"):
        assert check(**{name: None}) == BAD, name
    for name in ("n_rows", "nnz", "n_x", "n_coeffs"):                      # a count >= 2^32
        for big in (1 << 32, (1 << 32) + 5, 1 << 40):
            assert call(**{name: big}) == BAD, (name, big)
            assert check(**{name: big}) == BAD, (name, big)
    assert call(out=x) == BAD                                              # d_out == d_x
    assert call(n_rows=0) == 0                                             # nothing to do: succeeds, launches nothing
    assert call(n_rows=0, out=None, rp=None, nnz=0, col=None, cid=None, n_coeffs=0, cf=None, n_x=0, x=None) == 0
    assert lib.mi355zk_bn254_fr_from_repr_dev(None, x, 3, None) == BAD
    assert lib.mi355zk_bn254_fr_from_repr_dev(out, None, 3, None) == BAD
    assert lib.mi355zk_bn254_fr_from_repr_dev(None, None, 0, None) == 0


@pytest.mark.parametrize("which", ["small", "random"])
def test_compile_host_matches_prepare_prover(which):
    zk = _zk()
    circuit = K.small_circuit(zk) if which == "small" else K.random_circuit(zk)
    h = zk.circom._compile_host(circuit)
    n_c, n_in = len(circuit.constraints), circuit.num_inputs
    n = n_c + n_in
    exp = zk.circom.domain_exponent(n)
    m = 1 << exp
    assert (h["n"], h["exp"], h["m"]) == (n, exp, m) and (m // 2 < n <= m or n <= 1)
    rp, col, cid = h["row_ptr"], h["col"], h["coeff_id"]
    assert rp.dtype == col.dtype == cid.dtype == np.uint32 and h["coeffs"].dtype == np.uint64
    assert rp.shape == (3 * m + 1,) and rp[0] == 0 and rp[-1] == col.shape[0] == cid.shape[0]
    assert (np.diff(rp.astype(np.int64)) >= 0).all()
    table = K.from_limbs(h["coeffs"])
    assert len(set(table)) == len(table)                                   # one entry per distinct coefficient
    seen_empty = seen_repeat = seen_zero = seen_var0 = False
    for k in range(3):
        for i in range(m):
            b, e = int(rp[k * m + i]), int(rp[k * m + i + 1])
            if i < n_c:
                want = circuit.constraints[i][k]
            elif i < n:
                want = [(i - n_c, 1)] if k == 0 else []                    # x_i * 0 = 0
            else:
                want = []                                                  # the padding rows are empty
            assert [int(v) for v in col[b:e]] == [idx for idx, _ in want], (k, i)
            assert [table[int(t)] for t in cid[b:e]] == [c * K.MONT_R % K.R_ORDER for _, c in want], (k, i)
            if i < n_c:
                vs = [idx for idx, _ in want]
                seen_empty |= not want
                seen_repeat |= len(set(vs)) < len(vs)
                seen_zero |= any(c == 0 for _, c in want)
                seen_var0 |= 0 in vs
    if which == "random":
        assert seen_empty and seen_repeat and seen_zero and seen_var0      # the cases the circuit was built to contain
    ref = zk.circom.prepare_prover(circuit, "cpu")
    for name in ("a_aux_density", "b_input_density", "b_aux_density"):
        got, want = h[name], getattr(ref, name)
        gw, gn = got.words()
        ww, wn = want.words()
        assert gn == wn and np.array_equal(gw, ww), name
        assert got.get_total_density() == want.get_total_density(), name


def test_prepare_prover_dev_refuses_a_bad_witness_before_any_device_work():
    zk = _zk()
    circuit = K.small_circuit(zk)
    cc = zk.circom.CompiledCircuit(zk.circom._compile_host(circuit), "cpu")      # (host tensors: the refusals below come first)
    good = K.to_limbs(circuit.witness)
    for bad in (list(circuit.witness)[:-1], good[:-1], good[:, :3]):
        with pytest.raises(ValueError):
            zk.circom.prepare_prover_dev(cc, bad)
    for v in (K.R_ORDER, K.R_ORDER + 1, (1 << 256) - 1):                         # the array form holds canonical values
        bad = good.copy()
        bad[4] = K.to_limbs([v])[0]
        with pytest.raises(ValueError):
            zk.circom.prepare_prover_dev(cc, bad)
    assert zk.circom._all_below_r(K.to_limbs([0, 1, K.R_ORDER - 1, K.R_ORDER - (1 << 64)]))
