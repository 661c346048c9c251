"""groth16 `generate_parameters` (bellman/src/groth16/generator.rs:178-510) over the device library: a proving key from a circuit and
toxic waste, the step every test, benchmark and single-party user of the reference runs.

Its hot path is fixed-base scalar multiplication -- four G1 vectors and one G2 vector with one point per variable and the H query of
m - 1 points, all multiples of ONE generator -- which the reference does with `Wnaf::base(..).scalar(..)` window tables and this module
with bellman.FixedBaseTable.  The Fr side stays on the device as well: the powers of tau (mi355zk_bn254_fr_powers_dev), their inverse FFT
to the Lagrange coefficients at tau, and the per-variable evaluations of the QAP polynomials as ONE sparse product with a row per variable
(mi355zk_bn254_fr_sparse_matvec_dev), whose Montgomery results feed the table multiplications directly.

Host work is what it is in the reference: synthesising the circuit into per-variable term lists, a handful of field inversions and the six
single points of the verifying key.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import ceremony, circom
from . import lib as _lib
from .bellman import DeviceError, FixedBaseTable, SynthesisError, _stream_ptr

_R = ceremony._R_ORDER
_MONT_R = (1 << 256) % _R
_MONT_RINV = pow(_MONT_R, -1, _R)


def _mont(v: int) -> np.ndarray:
    return circom._limbs_array([v % _R * _MONT_R % _R])[0]


def _ptr(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _host_mul(group: int, base: np.ndarray, k: int):
    """k * base for one affine record through the library's host helpers (generator.rs:488-494: g1.mul(alpha).into_affine() ...)"""
    lib = _lib.load()
    limbs = 4 * group
    xyz = np.zeros(3 * limbs, dtype=np.uint64)
    if base.any():
        xyz[:2 * limbs] = base
        xyz[2 * limbs:2 * limbs + 4] = ceremony.G1_ONE_RAW[:4]   # Z = one (the Montgomery form of 1 in Fq: the generator's x)
    mul, to_affine = (lib.mi355zk_bn254_g1_mul, lib.mi355zk_bn254_g1_to_affine) if group == 1 else (lib.mi355zk_bn254_g2_mul, lib.mi355zk_bn254_g2_to_affine)
    out = np.zeros(2 * limbs, dtype=np.uint64)
    if mul(_ptr(xyz), _ptr(circom._limbs_array([k % _R])[0])) != 0 or to_affine(_ptr(out), _ptr(xyz)) != 0:
        raise ValueError("host scalar multiplication: bad arguments")
    return out


def _qap_matrix(cs, alpha: int, beta: int, gamma_inv: int, delta_inv: int) -> dict:
    """The per-variable term lists as ONE CSR matrix over the Lagrange coefficients (col = constraint index), inputs first, three row
    blocks of n_vars rows each: A_v, B_v and ext_v = (beta A_v + alpha B_v + C_v) * inv with inv = gamma^-1 on the input rows and delta^-1 on
    the aux rows.  An ext row is the concatenation of the variable's three term lists with the coefficients scaled by beta inv, alpha inv
    and inv on the host; the coefficients go through one table of distinct Montgomery values, as circom._compile_host's do."""
    at, bt, ct = cs.at_inputs + cs.at_aux, cs.bt_inputs + cs.bt_aux, cs.ct_inputs + cs.ct_aux
    n_vars = len(at)
    table = {}
    lens = np.zeros(3 * n_vars, dtype=np.int64)
    cols, ids = [], []

    def emit(row, terms, scale):
        lens[row] += len(terms)
        for coeff, lag in terms:
            cols.append(lag)
            ids.append(table.setdefault(coeff * scale % _R, len(table)))

    for v in range(n_vars):
        emit(v, at[v], 1)
    for v in range(n_vars):
        emit(n_vars + v, bt[v], 1)
    for v in range(n_vars):
        inv = gamma_inv if v < cs.num_inputs else delta_inv
        emit(2 * n_vars + v, at[v], beta * inv % _R)
        emit(2 * n_vars + v, bt[v], alpha * inv % _R)
        emit(2 * n_vars + v, ct[v], inv)
    row_ptr = np.zeros(3 * n_vars + 1, dtype=np.int64)
    np.cumsum(lens, out=row_ptr[1:])
    if int(row_ptr[-1]) >= 1 << 32 or len(table) >= 1 << 32:
        raise ValueError("the circuit has 2^32 terms or more")
    values = sorted(table, key=table.get)
    coeffs = circom._limbs_array(v * _MONT_R % _R for v in values) if values else np.zeros((0, 4), dtype=np.uint64)
    return {"n_vars": n_vars, "row_ptr": row_ptr.astype(np.uint32), "col": np.asarray(cols, dtype=np.uint32),
            "coeff_id": np.asarray(ids, dtype=np.uint32), "coeffs": coeffs}


def generate_parameters(circuit, g1, g2, alpha: int, beta: int, gamma: int, delta: int, tau: int, device):
    """generate_parameters (generator.rs:178-510): _queries below, and UnconstrainedVariable if an aux variable's L element is the point
    at infinity ("Don't allow any elements be unconstrained, so that the L query is always fully dense", :477-483)."""
    params = _queries(circuit, g1, g2, alpha, beta, gamma, delta, tau, device)
    l = params["l"]  # noqa: E741
    if l.shape[0] and bool((l == 0).all(dim=1).any().item()):
        raise SynthesisError(SynthesisError.UNCONSTRAINED_VARIABLE)
    return params


def _queries(circuit, g1, g2, alpha: int, beta: int, gamma: int, delta: int, tau: int, device):
    """Everything generate_parameters computes, before its UnconstrainedVariable test.  circuit: a circom.CircomCircuit; g1 / g2: raw affine records ((8,) / (16,) u64) of
    the generators -- non-infinite points of the order-r groups; alpha .. tau: ints mod r.  Returns the `params` dict that
    circom.mpc_parameters_new returns and circom.prove takes: {"vk": {alpha_g1, beta_g1, beta_g2, gamma_g2, delta_g1, delta_g2, ic}, "h",
    "l", "a", "b_g1", "b_g2"}, device records; a, b_g1 and b_g2 without their points at infinity (:505-508), h, l and ic as they are."""
    import torch

    lib = _lib.load()
    g1 = np.ascontiguousarray(np.asarray(g1, dtype=np.uint64).reshape(8))
    g2 = np.ascontiguousarray(np.asarray(g2, dtype=np.uint64).reshape(16))
    alpha, beta, gamma, delta, tau = (int(v) % _R for v in (alpha, beta, gamma, delta, tau))
    cs = circom.assemble(circuit)
    exp = circom.domain_exponent(cs.num_constraints)
    m = 1 << exp
    if gamma == 0 or delta == 0:
        raise SynthesisError(SynthesisError.UNEXPECTED_IDENTITY)
    device = torch.device(device)
    if device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    gamma_inv, delta_inv = pow(gamma, -1, _R), pow(delta, -1, _R)
    q = _qap_matrix(cs, alpha, beta, gamma_inv, delta_inv)
    n_vars = q["n_vars"]

    def check(rc, what):
        if rc == _lib.ERR_BAD_ARGS:
            raise ValueError(f"{what}: bad arguments")
        if rc != 0:
            raise DeviceError(f"mi355zk {what} rc={rc}")

    with torch.cuda.device(device):
        st = _stream_ptr()
        g1_table, g2_table = FixedBaseTable(g1, device), FixedBaseTable(g2, device)
        dptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        tau_m = _mont(tau)
        # powers of tau, and the H query g1^(tau^i t(tau) / delta), i < m - 1 (:248-304)
        powers = torch.empty((m, 4), dtype=torch.int64, device=device)
        check(lib.mi355zk_bn254_fr_powers_dev(dptr(powers), _ptr(tau_m), _ptr(_mont(1)), m, st), "fr_powers")
        z = np.zeros(4, dtype=np.uint64)
        check(lib.mi355zk_bn254_fr_domain_z(exp, _ptr(tau_m), _ptr(z)), "fr_domain_z")
        t_tau = int.from_bytes(z.tobytes(), "little") * _MONT_RINV % _R
        h_exp = torch.empty((m - 1, 4), dtype=torch.int64, device=device)
        check(lib.mi355zk_bn254_fr_powers_dev(dptr(h_exp), _ptr(tau_m), _ptr(_mont(t_tau * delta_inv)), m - 1, st), "fr_powers")
        h = g1_table.mul(h_exp, montgomery=True)
        # the Lagrange coefficients at tau (:311), then the QAP polynomials of every variable at tau (:324-473)
        check(lib.mi355zk_bn254_fr_domain_op_dev(dptr(powers), exp, _lib.OP_IFFT, st), "fr_domain_op")
        row_ptr, col, coeff_id = (torch.from_numpy(q[k].view(np.int32)).to(device) for k in ("row_ptr", "col", "coeff_id"))
        coeffs = torch.from_numpy(q["coeffs"].view(np.int64)).to(device)
        n_coeffs, nnz = int(q["coeffs"].shape[0]), int(q["col"].shape[0])
        check(lib.mi355zk_bn254_fr_sparse_matvec_check_dev(dptr(row_ptr), dptr(col), dptr(coeff_id), n_coeffs, m, 3 * n_vars, nnz, st),
              "fr_sparse_matvec_check")
        evals = torch.empty((3 * n_vars, 4), dtype=torch.int64, device=device)
        check(lib.mi355zk_bn254_fr_sparse_matvec_dev(dptr(evals), dptr(row_ptr), dptr(col), dptr(coeff_id), dptr(coeffs), n_coeffs, dptr(powers), m,
                                                     3 * n_vars, nnz, st), "fr_sparse_matvec")
        # A, B and IC / L queries (:406-426): a zero evaluation gives the all-zero record, which is what `if !at.is_zero()` leaves
        pts = g1_table.mul(evals, montgomery=True)
        a, b_g1, ext = pts[:n_vars], pts[n_vars:2 * n_vars], pts[2 * n_vars:]
        b_g2 = g2_table.mul(evals[n_vars:2 * n_vars].contiguous(), montgomery=True)
        ic, l = ext[:cs.num_inputs].contiguous(), ext[cs.num_inputs:].contiguous()  # noqa: E741
        point = lambda group, base, k: torch.from_numpy(_host_mul(group, base, k).view(np.int64).reshape(1, 8 * group)).to(device)  # noqa: E731
        vk = {"alpha_g1": point(1, g1, alpha), "beta_g1": point(1, g1, beta), "beta_g2": point(2, g2, beta), "gamma_g2": point(2, g2, gamma),
              "delta_g1": point(1, g1, delta), "delta_g2": point(2, g2, delta), "ic": ic}
        keep = lambda p: p[~(p == 0).all(dim=1)].contiguous()  # noqa: E731
        return {"vk": vk, "h": h, "l": l, "a": keep(a), "b_g1": keep(b_g1), "b_g2": keep(b_g2)}
