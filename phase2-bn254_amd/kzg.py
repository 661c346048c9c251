"""KZG polynomial commitments over a powers-of-tau accumulator: tau_g1[i] = tau^i G with tau_g2[1] = tau H is the structured reference
string, and commit / open / check are what a finished ceremony is used for.

The reference's tool set (bellman/src/sonic/util.rs), over its positive powers only (d = max, no negative powers):
  polynomial_commitment            :75-109    commit, commit_many      one multiexp per polynomial over srs["g1"]
  kate_divison                     :444-463   divide                   the suffix scan of csrc/fr_poly.hip, B points per call
  evaluate_at_consequitive_powers  :151-200   evaluate                 its first two launches
  polynomial_commitment_opening    :113-146   open, open_many          divide + ONE batched multiexp over the B quotients
  check_polynomial_commitment      :535-567   check, check_many        e(C - v G + z W, H) e(-W, tau H) == 1, all rows in one pairing launch

Conventions.  Coefficients are (n, 4) int64 device tensors of Montgomery Fr, lowest degree first, as EvaluationDomain holds them -- a
polynomial goes from an ifft to a commitment without leaving the device.  Points and values are Python ints mod r.  G1 / G2 elements are
raw affine records ((8,) / (16,) u64, host numpy for single results); the all-zero record is infinity, which is a valid commitment (the
zero polynomial) and a valid proof (a constant polynomial).  Built from the existing multiexp, sparse product and pairing: no group code
of its own.

The EVALUATION form (no counterpart in the reference; csrc/fr_inverse.hip, csrc/fr_evals.hip): a polynomial of degree < n = 2^log_n given by
evals[i] = p(omega^i), omega = the domain's generator, in natural order -- what EvaluationDomain.fft leaves and fr_sparse_matvec_dev writes --
commits over the Lagrange basis L_i(tau) G (srs_lagrange: one point ifft of the powers) and opens with one batch inversion of the
denominators omega^i - z instead of an ifft per polynomial:
  batch_inverse                    1 / a[i], zero for zero
  commit_evals, commit_evals_many  the same multiexps over lsrs["g1_lagrange"]
  evaluate_evals, divide_evals     p(z) (barycentric) and the quotient's evaluations, B points per call, z inside the domain included
  open_evals, open_evals_many      divide_evals + ONE batched multiexp over the Lagrange basis
The commitments and proofs are the group elements of commit / open, so check and check_many verify them as they are.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import ceremony, pairing
from . import lib as _lib
from . import prover as _prover
from .bellman import DeviceError, FullDensity, _stream_ptr, multiexp, multiexp_many

_R = ceremony._R_ORDER
_MONT_R = (1 << 256) % _R
_MONT_RINV = pow(_MONT_R, -1, _R)


def _mont_rows(vals) -> np.ndarray:
    """ints -> (len, 4) u64 Montgomery Fr"""
    buf = b"".join((int(v) % _R * _MONT_R % _R).to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


def _canon_rows(vals) -> np.ndarray:
    buf = b"".join((int(v) % _R).to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


def _ints(rows) -> list:
    """(k, 4) Montgomery Fr rows on the host -> ints"""
    rows = np.ascontiguousarray(rows).view(np.uint64).reshape(-1, 4)
    return [int.from_bytes(r.tobytes(), "little") * _MONT_RINV % _R for r in rows]


def _check(rc: int, what: str):
    if rc == _lib.ERR_BAD_ARGS:
        raise ValueError(f"{what}: bad arguments")
    if rc != 0:
        raise DeviceError(f"mi355zk {what} rc={rc}")


def _coeffs(coeffs):
    if not (getattr(coeffs, "is_cuda", False) and coeffs.dim() == 2 and coeffs.shape[1] == 4 and coeffs.element_size() == 8):
        raise ValueError("coefficients are an (n, 4) int64 device tensor of Montgomery Fr")
    return coeffs.contiguous()


def _points(zs) -> np.ndarray:
    zs = list(zs)
    if not 1 <= len(zs) <= _lib.POLY_MAX_POINTS:
        raise ValueError(f"between 1 and {_lib.POLY_MAX_POINTS} points per call")
    return _mont_rows(zs)


# ---- the structured reference string

def srs_from_points(g1_powers, g2_one, g2_tau) -> dict:
    """An SRS from the caller's own vectors: g1_powers (d + 1, 8) device tensor of tau^i G, g2_one = H and g2_tau = tau H ((16,) records)."""
    if g1_powers.dim() != 2 or g1_powers.shape[1] != 8 or g1_powers.shape[0] < 1 or g2_one.numel() != 16 or g2_tau.numel() != 16:
        raise ValueError("srs: g1_powers is (d + 1, 8), g2_one and g2_tau are G2 records")
    return {"g1": g1_powers, "g2_one": g2_one, "g2_tau": g2_tau}


def srs_from_accumulator(acc, degree=None) -> dict:
    """The SRS inside a powers-of-tau accumulator (ceremony.read_accumulator / contribute_accumulator): views of tau_g1[: degree + 1] and
    tau_g2[0], tau_g2[1], no copies.  degree None: every power the accumulator holds."""
    g1, g2 = acc["tau_g1"], acc["tau_g2"]
    degree = int(g1.shape[0]) - 1 if degree is None else int(degree)
    if degree < 0 or degree + 1 > int(g1.shape[0]) or int(g2.shape[0]) < 2:
        raise ValueError(f"the accumulator holds {int(g1.shape[0])} powers in G1 and {int(g2.shape[0])} in G2: too short for degree {degree}")
    return srs_from_points(g1[:degree + 1], g2[0], g2[1])


# ---- the Fr half: csrc/fr_poly.hip

def evaluate(coeffs, zs) -> list:
    """[p(z) for z in zs]: mi355zk_bn254_fr_poly_eval_dev, all points in one launch sequence"""
    import torch

    coeffs, z = _coeffs(coeffs), _points(zs)
    out = torch.empty((z.shape[0], 4), dtype=torch.int64, device=coeffs.device)
    with torch.cuda.device(coeffs.device):
        _check(_lib.load().mi355zk_bn254_fr_poly_eval_dev(C.c_void_p(out.data_ptr()), C.c_void_p(coeffs.data_ptr()), coeffs.shape[0],
                                                          z.ctypes.data_as(C.c_void_p), z.shape[0], _stream_ptr()), "fr_poly_eval")
    return _ints(out.cpu().numpy())


def divide(coeffs, zs):
    """p(x) = q_j(x) (x - z_j) + p(z_j) for every z_j: (q: (B, n - 1, 4) device tensor, [p(z_j)]) -- mi355zk_bn254_fr_poly_divide_dev"""
    import torch

    coeffs, z = _coeffs(coeffs), _points(zs)
    n, b = int(coeffs.shape[0]), int(z.shape[0])
    qn = max(n - 1, 0)
    q = torch.empty((b, qn, 4), dtype=torch.int64, device=coeffs.device)
    rem = torch.empty((b, 4), dtype=torch.int64, device=coeffs.device)
    with torch.cuda.device(coeffs.device):
        _check(_lib.load().mi355zk_bn254_fr_poly_divide_dev(C.c_void_p(q.data_ptr()) if qn else None, qn, C.c_void_p(rem.data_ptr()),
                                                            C.c_void_p(coeffs.data_ptr()) if n else None, n, z.ctypes.data_as(C.c_void_p), b,
                                                            _stream_ptr()), "fr_poly_divide")
    return q, _ints(rem.cpu().numpy())


# ---- the evaluation form, Fr half: csrc/fr_inverse.hip, csrc/fr_evals.hip

def batch_inverse(a, out=None, count_zeros=False):
    """1 / a[i] for any (..., 4) int64 device tensor of Montgomery Fr, zero where a[i] is zero: mi355zk_bn254_fr_batch_inverse_dev, one field
    inversion per call.  out: None (a new tensor), `a` itself (in place) or a tensor of a's shape that does not overlap it.  With count_zeros
    the result is (out, the number of zero elements), which waits for the device."""
    import torch

    if not (getattr(a, "is_cuda", False) and a.dim() >= 1 and a.shape[-1] == 4 and a.element_size() == 8 and a.is_contiguous()):
        raise ValueError("batch_inverse: a contiguous (..., 4) int64 device tensor of Montgomery Fr")
    if out is None:
        out = torch.empty_like(a)
    elif not (getattr(out, "is_cuda", False) and out.shape == a.shape and out.dtype == a.dtype and out.device == a.device and out.is_contiguous()):
        raise ValueError("batch_inverse: out has a's shape, dtype and device")
    n = a.numel() // 4
    with torch.cuda.device(a.device):
        zeros = torch.empty(1, dtype=torch.int32, device=a.device) if count_zeros else None
        _check(_lib.load().mi355zk_bn254_fr_batch_inverse_dev(C.c_void_p(out.data_ptr()) if n else None, C.c_void_p(a.data_ptr()) if n else None, n,
                                                              C.c_void_p(zeros.data_ptr()) if count_zeros else None, _stream_ptr()), "fr_batch_inverse")
    return (out, int(zeros.item()) & 0xFFFFFFFF) if count_zeros else out


def _evals(evals):
    evals = _coeffs(evals)
    n = int(evals.shape[0])
    if n == 0 or n & (n - 1):
        raise ValueError("evaluations over a domain: a power of two of them")
    return evals, n.bit_length() - 1


def _evals_divide(evals, zs, with_quotients: bool):
    import torch

    (evals, log_n), z = _evals(evals), _points(zs)
    n, b = 1 << log_n, int(z.shape[0])
    q = torch.empty((b, n, 4), dtype=torch.int64, device=evals.device) if with_quotients else None
    values = torch.empty((b, 4), dtype=torch.int64, device=evals.device)
    with torch.cuda.device(evals.device):
        _check(_lib.load().mi355zk_bn254_fr_evals_divide_dev(C.c_void_p(q.data_ptr()) if with_quotients else None, n, C.c_void_p(values.data_ptr()),
                                                             C.c_void_p(evals.data_ptr()), log_n, z.ctypes.data_as(C.c_void_p), b, _stream_ptr()),
               "fr_evals_divide")
    return q, _ints(values.cpu().numpy())


def evaluate_evals(evals, zs) -> list:
    """[p(z) for z in zs] from p's evaluations over the domain (barycentric; a z in the domain reads its evaluation)"""
    return _evals_divide(evals, zs, False)[1]


def divide_evals(evals, zs):
    """(q: (B, n, 4) device tensor, [p(z_j)]): q[j, i] = ((p(x) - p(z_j)) / (x - z_j))(omega^i) -- mi355zk_bn254_fr_evals_divide_dev"""
    return _evals_divide(evals, zs, True)


# ---- commitments

def _srs_bases(srs, n: int):
    g1 = srs["g1"]
    if n > int(g1.shape[0]):
        raise ValueError(f"a polynomial of {n} coefficients over an SRS of {int(g1.shape[0])} powers")
    return g1[:n]


def _to_affine_many(jacs) -> np.ndarray:
    """Jacobian limbs of the multiexps -> (B, 8) affine records"""
    return np.stack([_prover._to_affine(j) for j in jacs]) if len(jacs) else np.zeros((0, 8), dtype=np.uint64)


def commit(srs, coeffs) -> np.ndarray:
    """sum_i coeffs[i] tau^i G as an (8,) affine record: one multiexp, the Montgomery scalars converted inside it"""
    coeffs = _coeffs(coeffs)
    n = int(coeffs.shape[0])
    bases = _srs_bases(srs, n)
    if n == 0:
        return np.zeros(8, dtype=np.uint64)
    return _prover._to_affine(multiexp(None, (bases, 0), FullDensity(), coeffs, scalars_montgomery=True).wait())


def commit_many(srs, polys) -> np.ndarray:
    """commit for the B polynomials of a (B, n, 4) tensor: (B, 8) records from one batched multiexp"""
    if not (getattr(polys, "is_cuda", False) and polys.dim() == 3 and polys.shape[2] == 4):
        raise ValueError("polys is a (B, n, 4) int64 device tensor")
    polys = polys.contiguous()
    b, n = int(polys.shape[0]), int(polys.shape[1])
    bases = _srs_bases(srs, n)
    if n == 0 or b == 0:
        return np.zeros((b, 8), dtype=np.uint64)
    futures = multiexp_many(None, (bases, 0), FullDensity(), polys, scalars_montgomery=True)
    return _to_affine_many([f.wait() for f in futures])


def open_many(srs, coeffs, zs):
    """(values, proofs) of p at every z: proofs[j] = q_j(tau) G as (B, 8) records -- one divide with B points, one batched multiexp over
    srs["g1"][: n - 1], the affine conversions together"""
    coeffs = _coeffs(coeffs)
    bases = _srs_bases(srs, int(coeffs.shape[0]))
    q, values = divide(coeffs, zs)
    return values, commit_many({"g1": bases}, q)


def open(srs, coeffs, z):  # noqa: A001
    """(p(z), the (8,) proof record)"""
    values, proofs = open_many(srs, coeffs, [z])
    return values[0], proofs[0]


# ---- the evaluation form, group half

def srs_lagrange(srs, log_n: int) -> dict:
    """srs with "g1_lagrange" = L_i(tau) G for the domain of 2^log_n points (one point ifft of a copy of the first 2^log_n powers) and "log_n"."""
    n = 1 << int(log_n)
    g1 = srs["g1"]
    if n > int(g1.shape[0]):
        raise ValueError(f"a domain of {n} points over an SRS of {int(g1.shape[0])} powers")
    import torch

    with torch.cuda.device(g1.device):
        lagrange = ceremony.point_ifft(g1[:n].clone().contiguous())
    return {**srs, "g1_lagrange": lagrange, "log_n": int(log_n)}


def _lagrange_srs(lsrs, n: int) -> dict:
    if "g1_lagrange" not in lsrs or n != 1 << lsrs["log_n"]:
        raise ValueError(f"{n} evaluations need the Lagrange SRS of that domain (srs_lagrange)")
    return {"g1": lsrs["g1_lagrange"]}


def commit_evals(lsrs, evals) -> np.ndarray:
    """sum_i evals[i] L_i(tau) G: the (8,) record of commit(srs, ifft(evals))"""
    evals, _ = _evals(evals)
    return commit(_lagrange_srs(lsrs, int(evals.shape[0])), evals)


def commit_evals_many(lsrs, evals_b) -> np.ndarray:
    """commit_evals for the B polynomials of a (B, n, 4) tensor: one batched multiexp"""
    if not (getattr(evals_b, "is_cuda", False) and evals_b.dim() == 3 and evals_b.shape[2] == 4):
        raise ValueError("evals is a (B, n, 4) int64 device tensor")
    return commit_many(_lagrange_srs(lsrs, int(evals_b.shape[1])), evals_b)


def open_evals_many(lsrs, evals, zs):
    """(values, proofs) of p at every z, from p's evaluations: one evals_divide with B points, one batched multiexp over the Lagrange basis"""
    evals, _ = _evals(evals)
    bases = _lagrange_srs(lsrs, int(evals.shape[0]))
    q, values = divide_evals(evals, zs)
    return values, commit_many(bases, q)


def open_evals(lsrs, evals, z):
    """(p(z), the (8,) proof record): what open gives for ifft(evals)"""
    values, proofs = open_evals_many(lsrs, evals, [z])
    return values[0], proofs[0]


def check_many(srs, commitments, zs, values, proofs) -> np.ndarray:
    """ok[i] = e(C_i - v_i G + z_i W_i, H) e(-W_i, tau H) == 1 as a numpy bool vector.  The n points F_i = C_i - v_i G + z_i W_i are ONE sparse
    product of three terms per row over [G, C.., W..], the 2 n pairings ONE launch over n two-pair groups (F_i, H), (W_i, -tau H) -- the
    same product with the sign moved to tau H: one host negation per call instead of n.  An infinite W (constant polynomial) or C (zero
    polynomial) is a point like any other here, which is why this is not same_ratio_batch."""
    import torch

    dev = srs["g1"].device
    rec = lambda x: pairing._records(x, 8)  # noqa: E731
    cs, ws = rec(commitments), rec(proofs)
    zs, values = [int(z) % _R for z in zs], [int(v) % _R for v in values]
    n = len(zs)
    if not (cs.shape[0] == ws.shape[0] == len(values) == n):
        raise ValueError("check_many: one commitment, point, value and proof per row")
    if n == 0:
        return np.zeros(0, dtype=bool)
    to_dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else a.dtype)).to(dev)  # noqa: E731
    with torch.cuda.device(dev):
        w_dev = to_dev(ws)
        bases = torch.cat([srs["g1"][:1], to_dev(cs), w_dev]).contiguous()
        idx = np.arange(n, dtype=np.int32)
        col = np.stack([np.zeros(n, dtype=np.int32), 1 + idx, 1 + n + idx], axis=1).reshape(-1)
        coeff = np.stack([_canon_rows([_R - v for v in values]), _canon_rows([1] * n), _canon_rows(zs)], axis=1).reshape(-1, 4)
        row_ptr = np.arange(0, 3 * n + 1, 3, dtype=np.int32)
        f = ceremony.eval_qap(bases, to_dev(row_ptr), to_dev(col), to_dev(coeff))
        h = srs["g2_one"].reshape(1, 16).to(dev)
        neg_tau_h = to_dev(pairing._neg_record(pairing._records(srs["g2_tau"], 16)[0]).reshape(1, 16))
        g1 = torch.stack([f, w_dev], dim=1).reshape(2 * n, 8)
        g2 = torch.cat([h, neg_tau_h]).repeat(n, 1)
        gt = pairing.pairing_product(g1, g2, to_dev(np.arange(0, 2 * n + 1, 2, dtype=np.int32)))
        return pairing.gt_eq(gt).cpu().numpy()


def check(srs, commitment, z, value, proof) -> bool:
    """check_polynomial_commitment for one opening: check_many with one row"""
    return bool(check_many(srs, pairing._records(commitment, 8), [z], [value], pairing._records(proof, 8))[0])
