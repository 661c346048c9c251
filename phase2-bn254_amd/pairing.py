"""The checking half of the reference over the device pairing (include/mi355zk.h: mi355zk_bn254_pairing_product_dev): every verification
path of the reference ends in a BN254 pairing, and the batched forms -- all same_ratio checks of a transcript, many proofs -- are one
launch here, one lane per Miller loop.

Mirrored interfaces (same names, argument meaning and order):
  pairing/src/lib.rs:101              Engine::pairing(p, q)
  pairing/src/bn256/mod.rs:57-226     Engine::miller_loop + final_exponentiation  -> miller_loop_product(pairs)
  powersoftau/src/utils.rs:151-159    same_ratio(g1, g2)  (phase2/src/utils.rs:35 is the same function)
  bellman/src/groth16/verifier.rs     prepare_verifying_key(vk), verify_proof(pvk, proof, public_inputs)

Data.  Points are raw affine records of u64 limbs (8 per G1 point, 16 per G2 point, the all-zero record = infinity); a GT value is 48
u64 limbs (384 B), a unique fully reduced Fq12 element, so equality of values is equality of bytes.  Host records (numpy) go through the
library's single-thread host product, device tensors (torch, int64 holding the limbs) through the kernels on the current stream.
DOMAIN: G1 points on the curve, G2 points in the order-r subgroup -- the reference tests neither, and neither does this module;
ceremony.g2_subgroup_check establishes it for G2 data from outside.  verify_proofs_batch is the exception: its random linear combination
is sound only for B in the order-r subgroup (a B with a cofactor component can cancel in the weighted product), so it runs that check
itself unless told otherwise.

Beyond the reference (one verifying key, many proofs, nothing per proof on the host): prepare_verifying_key_dev, input_accumulators,
verify_proofs_dev, batch_pairs / verify_proofs_batch, and read_proofs / write_proofs for the wire format of groth16/mod.rs:42-90.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _lib
from . import prover as _prover
from .bellman import DeviceError, SynthesisError, _stream_ptr

_Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583   # fq.rs:5
GT_WORDS = 48
GT_ONE = np.zeros(GT_WORDS, dtype=np.uint64)
GT_ONE[:4] = [(((1 << 256) % _Q) >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]   # c0.c0.c0 = the Montgomery form of 1


def _check(rc: int, what: str):
    if rc == _lib.ERR_BAD_ARGS:
        raise ValueError(f"{what}: bad arguments")
    if rc != 0:
        raise DeviceError(f"mi355zk {what} rc={rc}")


def _hp(a: np.ndarray):
    return a.ctypes.data_as(C.c_void_p)


def _dp(t):
    return C.c_void_p(t.data_ptr())


def _on_device(x) -> bool:
    return bool(getattr(x, "is_cuda", False))


def _records(x, width: int) -> np.ndarray:
    """host records as one contiguous (n, width) u64 array (device tensors are downloaded)"""
    if hasattr(x, "cpu"):
        x = x.cpu().numpy()
    a = np.asarray(x)
    if a.dtype != np.uint64:
        a = a.view(np.uint64) if a.dtype == np.int64 else a.astype(np.uint64)
    return np.ascontiguousarray(a.reshape(-1, width))


def pairing_product(g1, g2, group_ptr=None):
    """out[g] = final_exponentiation(prod over the pairs i of group g of miller(g1[i], g2[i])) on the device: g1 (n, 8), g2 (n, 16) int64
    device tensors; group_ptr: (n_groups + 1,) int32 device tensor, nondecreasing from 0 to n (None: every pair is its own group).
    Returns (n_groups, 48) int64.  Asynchronous on the current stream."""
    import torch

    n = int(g1.shape[0])
    if g1.dim() != 2 or g2.dim() != 2 or g1.shape[1] != 8 or g2.shape[1] != 16 or int(g2.shape[0]) != n:
        raise ValueError("pairing_product: g1 is (n, 8), g2 (n, 16) raw affine records")
    g1, g2 = g1.contiguous(), g2.contiguous()
    if group_ptr is None:
        n_groups, ptr = n, None
    else:
        if group_ptr.dtype != torch.int32 or group_ptr.dim() != 1 or group_ptr.shape[0] < 1:
            raise ValueError("pairing_product: group_ptr is an int32 vector of n_groups + 1 entries")
        group_ptr = group_ptr.contiguous()
        n_groups, ptr = int(group_ptr.shape[0]) - 1, _dp(group_ptr)
    out = torch.empty((n_groups, GT_WORDS), dtype=torch.int64, device=g1.device)
    with torch.cuda.device(g1.device):
        _check(_lib.load().mi355zk_bn254_pairing_product_dev(_dp(out), _dp(g1), _dp(g2), n, ptr, n_groups, _stream_ptr()), "pairing_product")
    return out


def gt_eq(a, b=None):
    """flags[i] = a[i] == b[i] (b None: a[i] is one) for (n, 48) device tensors -> (n,) bool device tensor"""
    import torch

    n = int(a.shape[0])
    flags = torch.empty(n, dtype=torch.uint8, device=a.device)
    lib = _lib.load()
    with torch.cuda.device(a.device):
        if b is None:
            _check(lib.mi355zk_bn254_gt_is_one_dev(_dp(flags), _dp(a.contiguous()), n, _stream_ptr()), "gt_is_one")
        else:
            _check(lib.mi355zk_bn254_gt_eq_dev(_dp(flags), _dp(a.contiguous()), _dp(b.contiguous()), n, _stream_ptr()), "gt_eq")
    return flags.bool()


def miller_loop_product(pairs):
    """final_exponentiation(miller_loop(pairs)) for a sequence of (p, q) records: ONE GT value.  Host records -> (48,) u64 numpy through the
    library's host product (no device needed); device tensors -> (48,) int64 device tensor through the kernels."""
    import_torch = any(_on_device(p) or _on_device(q) for p, q in pairs)
    if import_torch:
        import torch

        dev = next(x.device for pq in pairs for x in pq if _on_device(x))
        g1 = torch.cat([p.reshape(1, 8).to(dev) for p, _ in pairs])
        g2 = torch.cat([q.reshape(1, 16).to(dev) for _, q in pairs])
        ptr = torch.tensor([0, len(pairs)], dtype=torch.int32, device=dev)
        return pairing_product(g1, g2, ptr)[0]
    n = len(pairs)
    g1 = np.concatenate([_records(p, 8) for p, _ in pairs]) if n else np.zeros((0, 8), np.uint64)
    g2 = np.concatenate([_records(q, 16) for _, q in pairs]) if n else np.zeros((0, 16), np.uint64)
    if g1.shape[0] != n or g2.shape[0] != n:
        raise ValueError("miller_loop_product: one G1 and one G2 record per pair")
    out = np.zeros(GT_WORDS, dtype=np.uint64)
    _check(_lib.load().mi355zk_bn254_pairing_product(_hp(out), _hp(g1), _hp(g2), n), "pairing_product (host)")
    return out


def pairing(p, q):
    """Engine::pairing (pairing/src/lib.rs:101): e(p, q)"""
    return miller_loop_product([(p, q)])


def _gt_equal(a, b) -> bool:
    if _on_device(a) or _on_device(b):
        return bool((a == b).all().item())
    return bool(np.array_equal(a, b))


def _is_zero(x) -> bool:
    return not bool((x != 0).any())


def same_ratio(g1_pair, g2_pair) -> bool:
    """utils.rs:151-159: e(g1.0, g2.1) == e(g1.1, g2.0), False if any of the four points is zero"""
    if any(_is_zero(x) for x in (*g1_pair, *g2_pair)):
        return False
    return _gt_equal(pairing(g1_pair[0], g2_pair[1]), pairing(g1_pair[1], g2_pair[0]))


def same_ratio_batch(g1_a, g1_b, g2_a, g2_b) -> np.ndarray:
    """same_ratio((g1_a[i], g1_b[i]), (g2_a[i], g2_b[i])) for every i: (n, 8) / (n, 16) device tensors -> (n,) numpy bool.  One launch over
    2 n single-pair groups -- e(g1_a[i], g2_b[i]) then e(g1_b[i], g2_a[i]) -- and one comparison kernel."""
    import torch

    n = int(g1_a.shape[0])
    if not (int(g1_b.shape[0]) == int(g2_a.shape[0]) == int(g2_b.shape[0]) == n):
        raise ValueError("same_ratio_batch: four vectors of one length")
    if n == 0:
        return np.zeros(0, dtype=bool)
    gt = pairing_product(torch.cat([g1_a, g1_b]), torch.cat([g2_b, g2_a]))
    zero = lambda t: (t == 0).all(dim=1)  # noqa: E731
    ok = gt_eq(gt[:n], gt[n:]) & ~(zero(g1_a) | zero(g1_b) | zero(g2_a) | zero(g2_b))
    return ok.cpu().numpy()


def _neg_record(rec: np.ndarray) -> np.ndarray:
    """-(x, y) = (x, -y) on a raw affine record: each Fq limb group of y becomes q - y (Montgomery forms negate like the values)"""
    rec = np.array(rec, dtype=np.uint64).reshape(-1)
    if not rec.any():
        return rec
    half = rec.size // 2
    for k in range(half // 4):
        sl = slice(half + 4 * k, half + 4 * k + 4)
        v = sum(int(x) << (64 * i) for i, x in enumerate(rec[sl]))
        rec[sl] = _prover._limbs((_Q - v) % _Q)
    return rec


def prepare_verifying_key(vk) -> dict:
    """verifier.rs:19-34 over the `vk` dict of generator.generate_parameters / circom.mpc_parameters_new: alpha_g1_beta_g2 = e(alpha_g1,
    beta_g2) (the one pairing per key: the host product), neg_gamma_g2, neg_delta_g2 and ic, all host records."""
    alpha, beta = _records(vk["alpha_g1"], 8)[0], _records(vk["beta_g2"], 16)[0]
    return {"alpha_g1_beta_g2": pairing(alpha, beta), "neg_gamma_g2": _neg_record(_records(vk["gamma_g2"], 16)[0]),
            "neg_delta_g2": _neg_record(_records(vk["delta_g2"], 16)[0]), "ic": _records(vk["ic"], 8)}


def _input_accumulator(pvk, public_inputs) -> np.ndarray:
    """ic[0] + sum_i public_inputs[i] * ic[i + 1] (verifier.rs:44-48), affine; the MalformedVerifyingKey test of :40-42"""
    ic = pvk["ic"]
    if len(public_inputs) + 1 != ic.shape[0]:
        raise SynthesisError(SynthesisError.MALFORMED_VERIFYING_KEY)
    acc = _prover._from_affine(ic[0])
    for x, base in zip(public_inputs, ic[1:]):
        acc = _prover._add(acc, _prover._mul(base, int(x)))
    return _prover._to_affine(acc)


def verify_proofs(pvk, proofs, public_inputs, device=None) -> np.ndarray:
    """verify_proof for n proofs against one key as n three-pair groups in ONE launch: proofs[i] = (a, b, c) raw affine records as
    prover.create_proof returns them, public_inputs[i] that proof's inputs (ints mod r, without the leading one).  -> (n,) numpy bool."""
    import torch

    if len(proofs) != len(public_inputs):
        raise ValueError("verify_proofs: one list of public inputs per proof")
    accs = [_input_accumulator(pvk, inputs) for inputs in public_inputs]   # raises before any device work
    n = len(proofs)
    if n == 0:
        return np.zeros(0, dtype=bool)
    g1 = np.zeros((3 * n, 8), dtype=np.uint64)
    g2 = np.zeros((3 * n, 16), dtype=np.uint64)
    for i, ((a, b, c), acc) in enumerate(zip(proofs, accs)):
        g1[3 * i], g1[3 * i + 1], g1[3 * i + 2] = _records(a, 8)[0], acc, _records(c, 8)[0]
        g2[3 * i], g2[3 * i + 1], g2[3 * i + 2] = _records(b, 16)[0], pvk["neg_gamma_g2"], pvk["neg_delta_g2"]
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    ptr = torch.arange(0, 3 * n + 1, 3, dtype=torch.int32, device=device)
    gt = pairing_product(torch.from_numpy(g1.view(np.int64)).to(device), torch.from_numpy(g2.view(np.int64)).to(device), ptr)
    want = torch.from_numpy(np.ascontiguousarray(pvk["alpha_g1_beta_g2"]).view(np.int64)).to(device).reshape(1, GT_WORDS).expand(n, GT_WORDS)
    return gt_eq(gt, want).cpu().numpy()


def verify_proof(pvk, proof, public_inputs, device=None) -> bool:
    """verifier.rs:36-67: e(A, B) e(acc, -gamma) e(C, -delta) == e(alpha, beta) as one three-pair product on the device.  Raises
    SynthesisError(MALFORMED_VERIFYING_KEY) when len(public_inputs) + 1 != len(ic), before any device work."""
    return bool(verify_proofs(pvk, [proof], [public_inputs], device)[0])


# ---------------------------------------------------------------------------------------------------------------
# Many proofs against ONE verifying key, on the device from the public inputs to the verdicts.  The input accumulators are one launch
# over the window tables of ic[1:] (mi355zk_bn254_g1_fixed_bases_lincomb_dev, one lane per proof); the batch check folds the n checks into
# n + 3 Miller loops and one final exponentiation with random weights.
_R = _prover._R_ORDER


class FixedBasesTable:
    """Window tables of SEVERAL G1 bases laid end to end (mi355zk_bn254_g1_fixed_bases_build_dev).  bases: (n_bases, 8) u64 host records on
    the curve, the all-zero record allowed; anything else raises ValueError.  lincomb(scalars, first) returns first + sum_j scalars[i][j] *
    bases[j] for every row i as an (n, 8) int64 device tensor, asynchronous on the current stream."""

    def __init__(self, bases, device=None):
        import torch

        bases = np.ascontiguousarray(_records(bases, 8))
        lib = _lib.load()
        self.n_bases = int(bases.shape[0])
        nbytes = int(lib.mi355zk_fixed_bases_table_bytes(self.n_bases))
        if self.n_bases and nbytes == 0:
            raise ValueError("fixed_bases_build: too many bases")
        self.device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.table = torch.empty(nbytes // 8, dtype=torch.int64, device=self.device)   # (the entry format is the library's own)
        with torch.cuda.device(self.device):
            rc = lib.mi355zk_bn254_g1_fixed_bases_build_dev(_dp(self.table), nbytes, _hp(bases), self.n_bases, _stream_ptr())
        if rc == _lib.ERR_BAD_ARGS:
            raise ValueError("fixed_bases_build: a base is not on the curve")
        _check(rc, "fixed_bases_build")

    def lincomb(self, scalars, first=None, slice_len: int = 0):
        """scalars: (n, n_bases, 4) int64 device tensor of canonical FrRepr; first: one (8,) device record or None (the identity);
        slice_len: bases per lane, 0 = the library's plan (mi355zk_fixed_bases_plan)"""
        import torch

        n = int(scalars.shape[0])
        if scalars.dtype != torch.int64 or scalars.device != self.device or scalars.numel() != n * self.n_bases * 4:
            raise ValueError("lincomb: scalars are an (n, n_bases, 4) int64 tensor on the table's device")
        scalars = scalars.contiguous()
        if first is not None:
            first = first.reshape(8).contiguous()
        out = torch.empty((n, 8), dtype=torch.int64, device=self.device)
        with torch.cuda.device(self.device):
            _check(_lib.load().mi355zk_bn254_g1_fixed_bases_lincomb_dev(_dp(out), _dp(self.table), self.n_bases, None if first is None else _dp(first),
                                                                        _dp(scalars), n, slice_len, _stream_ptr()), "fixed_bases_lincomb")
        return out


def prepare_verifying_key_dev(vk, device=None) -> dict:
    """prepare_verifying_key(vk), plus what the device paths below keep in HBM, under "dev": the table set over ic[1:] ("ic_tables": the input
    accumulators), a second set over ALL of ic ("ic_all_tables": the batch check's one combination, cut into slices) and one over alpha_g1
    ("alpha_table"), the records ic[0], alpha_g1, beta_g2, -gamma, -delta and the GT target e(alpha, beta)."""
    import torch

    pvk = prepare_verifying_key(vk)
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(device)  # noqa: E731
    ic = pvk["ic"]
    alpha = _records(vk["alpha_g1"], 8)
    pvk["dev"] = {"device": device, "ic_tables": FixedBasesTable(ic[1:], device), "ic_all_tables": FixedBasesTable(ic, device),
                  "alpha_table": FixedBasesTable(alpha, device), "ic0": up(ic[0]), "alpha_g1": up(alpha[0]),
                  "beta_g2": up(_records(vk["beta_g2"], 16)[0]), "neg_gamma_g2": up(pvk["neg_gamma_g2"]), "neg_delta_g2": up(pvk["neg_delta_g2"]),
                  "alpha_g1_beta_g2": up(pvk["alpha_g1_beta_g2"])}
    return pvk


def _inputs_dev(pvk, public_inputs):
    """the public inputs of n proofs as an (n, l, 4) int64 device tensor of canonical FrRepr; the MalformedVerifyingKey test of
    verifier.rs:40-42 before any device work"""
    import torch

    n_ic, device = int(pvk["ic"].shape[0]), pvk["dev"]["device"]
    if hasattr(public_inputs, "is_cuda"):
        if public_inputs.dim() != 3 or int(public_inputs.shape[2]) != 4 or int(public_inputs.shape[1]) + 1 != n_ic:
            raise SynthesisError(SynthesisError.MALFORMED_VERIFYING_KEY)
        return public_inputs.to(device).contiguous()
    if isinstance(public_inputs, np.ndarray) and public_inputs.ndim == 3:
        if public_inputs.shape[2] != 4 or public_inputs.shape[1] + 1 != n_ic:
            raise SynthesisError(SynthesisError.MALFORMED_VERIFYING_KEY)
        arr = np.ascontiguousarray(public_inputs, dtype=np.uint64)
    else:
        rows = [list(row) for row in public_inputs]
        if any(len(row) + 1 != n_ic for row in rows):
            raise SynthesisError(SynthesisError.MALFORMED_VERIFYING_KEY)
        arr = np.zeros((len(rows), n_ic - 1, 4), dtype=np.uint64)
        for i, row in enumerate(rows):
            for j, x in enumerate(row):
                arr[i, j] = _prover._limbs(int(x) % _R)
    return torch.from_numpy(arr.view(np.int64)).to(device)


def input_accumulators(pvk, public_inputs):
    """ic[0] + sum_j public_inputs[i][j] * ic[j + 1] (verifier.rs:44-48) for every proof i in ONE launch over the key's window tables:
    (n, 8) int64 device tensor.  pvk: prepare_verifying_key_dev; public_inputs: ints mod r as nested lists, an (n, l, 4) u64 numpy array or
    an (n, l, 4) int64 device tensor of canonical FrRepr.  Raises SynthesisError(MALFORMED_VERIFYING_KEY) when l + 1 != len(ic), before any
    device work; l == 0 gives ic[0] n times."""
    x = _inputs_dev(pvk, public_inputs)
    return pvk["dev"]["ic_tables"].lincomb(x, pvk["dev"]["ic0"])


def _proofs_dev(pvk, proofs):
    """(a, b, c) device tensors of n records each, from that form or from the list form of verify_proofs"""
    import torch

    device = pvk["dev"]["device"]
    if isinstance(proofs, tuple) and len(proofs) == 3 and all(hasattr(p, "is_cuda") for p in proofs):
        a, b, c = (p.to(device).contiguous() for p in proofs)
    else:
        cols = [np.zeros((len(proofs), w), dtype=np.uint64) for w in (8, 16, 8)]
        for i, proof in enumerate(proofs):
            for col, rec, w in zip(cols, proof, (8, 16, 8)):
                col[i] = _records(rec, w)[0]
        a, b, c = (torch.from_numpy(col.view(np.int64)).to(device) for col in cols)
    if a.dim() != 2 or a.shape[1] != 8 or b.dim() != 2 or b.shape[1] != 16 or c.shape != a.shape or b.shape[0] != a.shape[0]:
        raise ValueError("proofs: a (n, 8), b (n, 16), c (n, 8) raw affine records")
    return a, b, c


def verify_proofs_dev(pvk, proofs, public_inputs) -> np.ndarray:
    """verify_proofs with nothing per proof on the host: one accumulator launch, one pairing launch over n three-pair groups, one gt_eq.
    pvk: prepare_verifying_key_dev; proofs: (a, b, c) device tensors of n records each, or the list verify_proofs takes; public_inputs as
    input_accumulators takes them.  -> (n,) numpy bool, the verdicts of verify_proofs (an all-zero record contributes one to its product)."""
    import torch

    x = _inputs_dev(pvk, public_inputs)                       # raises before any device work
    a, b, c = _proofs_dev(pvk, proofs)
    n, d = int(a.shape[0]), pvk["dev"]
    if int(x.shape[0]) != n:
        raise ValueError("verify_proofs_dev: one row of public inputs per proof")
    if n == 0:
        return np.zeros(0, dtype=bool)
    with torch.cuda.device(d["device"]):
        acc = d["ic_tables"].lincomb(x, d["ic0"])
        g1 = torch.stack([a, acc, c], dim=1).reshape(3 * n, 8)
        g2 = torch.stack([b, d["neg_gamma_g2"].expand(n, 16), d["neg_delta_g2"].expand(n, 16)], dim=1).reshape(3 * n, 16)
        ptr = torch.arange(0, 3 * n + 1, 3, dtype=torch.int32, device=d["device"])
        gt = pairing_product(g1, g2, ptr)
        return gt_eq(gt, d["alpha_g1_beta_g2"].reshape(1, GT_WORDS).expand(n, GT_WORDS)).cpu().numpy()


def _weighted_sums(x, r):
    """s_0 = sum_i r_i, s_j = sum_i r_i x[i][j - 1] (j = 1 .. l) and -s_0, mod r, on the device: (l + 2, 4) canonical FrRepr.  One sparse
    matrix-vector product (mi355zk_bn254_fr_sparse_matvec_dev) over the transposed inputs: row j's term i has the column i (the vector is r)
    and the coefficient x[i][j - 1]; rows 0 and l + 1 use the constants 1 and -1."""
    import torch

    lib = _lib.load()
    n, l, dev = int(x.shape[0]), int(x.shape[1]), x.device
    st = _stream_ptr()
    consts = torch.from_numpy(np.stack([_prover._limbs(1), _prover._limbs(_R - 1)]).view(np.int64)).to(dev)
    coeffs = torch.cat([x.reshape(n * l, 4), consts])         # canonical; made Montgomery in place below
    vec = r.clone()
    _check(lib.mi355zk_bn254_fr_from_repr_dev(_dp(coeffs), _dp(coeffs), n * l + 2, st), "fr_from_repr")
    _check(lib.mi355zk_bn254_fr_from_repr_dev(_dp(vec), _dp(vec), n, st), "fr_from_repr")
    i = torch.arange(n, dtype=torch.int32, device=dev)
    j = torch.arange(l, dtype=torch.int32, device=dev)
    coeff_id = torch.cat([torch.full((n,), n * l, dtype=torch.int32, device=dev), (i.reshape(1, n) * l + j.reshape(l, 1)).reshape(-1),
                          torch.full((n,), n * l + 1, dtype=torch.int32, device=dev)]).contiguous()
    col = i.repeat(l + 2).contiguous()
    row_ptr = torch.arange(0, (l + 2) * n + 1, n, dtype=torch.int32, device=dev)
    out = torch.empty((l + 2, 4), dtype=torch.int64, device=dev)
    _check(lib.mi355zk_bn254_fr_sparse_matvec_dev(_dp(out), _dp(row_ptr), _dp(col), _dp(coeff_id), _dp(coeffs), n * l + 2, _dp(vec), n, l + 2,
                                                  (l + 2) * n, st), "fr_sparse_matvec")
    _check(lib.mi355zk_bn254_fr_into_repr_dev(_dp(out), _dp(out), l + 2, st), "fr_into_repr")
    return out


def batch_pairs(pvk, proofs, public_inputs, key, coefficients=None):
    """The n + 3 pairs of the batch check with the weights r = ceremony.fr_random(n, key, stream_id=0) (or `coefficients`, an (n, 4) device
    tensor of canonical FrRepr): pair i < n is (r_i A_i, B_i), then (T, -gamma), (sum_i r_i C_i, -delta) and (-s_0 alpha, beta) with
    s_0 = sum_i r_i, s_j = sum_i r_i x[i][j] mod r and T = s_0 ic[0] + sum_j s_j ic[j].  The product of the pairs is one iff
    prod_i (e(A_i, B_i) e(acc_i, -gamma) e(C_i, -delta) e(alpha, beta)^-1)^r_i is.  r_i A_i: batch_exp; sum r_i C_i: the device multiexp; the s_j:
    one sparse matrix-vector product; T and s_0 alpha: the fixed-bases combination with one row.  Nothing on the host grows with n.
    -> (g1 (n + 3, 8), g2 (n + 3, 16)) int64 device tensors.  DOMAIN: the A, B, C records are not the identity (the multiexp refuses such
    bases) and every B lies in the order-r subgroup; verify_proofs_batch tests both."""
    import torch

    from . import ceremony

    x = _inputs_dev(pvk, public_inputs)
    a, b, c = _proofs_dev(pvk, proofs)
    n, d = int(a.shape[0]), pvk["dev"]
    if int(x.shape[0]) != n:
        raise ValueError("batch_pairs: one row of public inputs per proof")
    with torch.cuda.device(d["device"]):
        r = ceremony.fr_random(n, key, stream_id=0, device=d["device"]) if coefficients is None else coefficients.to(d["device"]).contiguous()
        if tuple(r.shape) != (n, 4):
            raise ValueError("batch_pairs: one coefficient per proof")
        ra = ceremony.batch_exp(a, r) if n else a
        l = int(x.shape[1])
        s = _weighted_sums(x, r) if n else torch.zeros((l + 2, 4), dtype=torch.int64, device=d["device"])
        t = d["ic_all_tables"].lincomb(s[:l + 1].reshape(1, l + 1, 4))
        neg_s0_alpha = d["alpha_table"].lincomb(s[l + 1:].reshape(1, 1, 4))
        sum_c = np.zeros(8, dtype=np.uint64)
        if n:
            sum_c = _prover._to_affine(ceremony.dense_multiexp(c, r))
        sum_c = torch.from_numpy(sum_c.view(np.int64)).to(d["device"]).reshape(1, 8)
        g1 = torch.cat([ra, t, sum_c, neg_s0_alpha])
        g2 = torch.cat([b, d["neg_gamma_g2"].reshape(1, 16), d["neg_delta_g2"].reshape(1, 16), d["beta_g2"].reshape(1, 16)])
    return g1, g2


def verify_proofs_batch(pvk, proofs, public_inputs, key=None, check_g2_subgroup: bool = True) -> bool:
    """The standard batch check of n proofs against one key: True iff the product over the ONE group of batch_pairs is one -- n + 3 Miller
    loops and one final exponentiation against the 3 n loops and n exponentiations of verify_proofs_dev.  The weights come from the stream
    of `key` (32 bytes; None: os.urandom), so a batch with a false proof passes with probability 2^-253.  False without a pairing when an A, B
    or C record is all zero (Proof::read, groth16/mod.rs:55-90, refuses such a proof) or, with check_g2_subgroup, when a B fails
    ceremony.g2_subgroup_check: the weighted combination is sound ONLY for B in the order-r subgroup, so check_g2_subgroup=False is for
    proofs whose B the caller has tested already.  False names no culprit: the caller then runs verify_proofs_dev over the same proofs --
    no second pass is hidden here."""
    import os

    from . import ceremony

    x = _inputs_dev(pvk, public_inputs)
    a, b, c = _proofs_dev(pvk, proofs)
    if int(a.shape[0]) == 0:
        return True
    zero = lambda t: bool((t == 0).all(dim=1).any().item())  # noqa: E731
    if zero(a) or zero(b) or zero(c):
        return False
    if check_g2_subgroup and ceremony.g2_subgroup_check(b) != -1:
        return False
    key = os.urandom(32) if key is None else key
    g1, g2 = batch_pairs(pvk, (a, b, c), x, key)
    import torch

    ptr = torch.tensor([0, int(g1.shape[0])], dtype=torch.int32, device=g1.device)
    return bool(gt_eq(pairing_product(g1, g2, ptr))[0].item())


def read_proofs(data):
    """n proofs on the wire (groth16/mod.rs:42-52: compressed A 32 B, B 64 B, C 32 B) as one uint8 device tensor of 128 n bytes -> (a, b, c)
    raw affine device records through the checked compressed decoder.  Raises ceremony.GroupDecodingError carrying the index of the PROOF
    whose point does not decode, and ceremony.DeserializationError for the point at infinity (mod.rs:55-90)."""
    from . import ceremony

    if data.numel() % 128:
        raise ValueError("read_proofs: 128 bytes per proof")
    rows = data.reshape(-1, 128)
    out = []
    for name, lo, hi, group in (("a", 0, 32, 1), ("b", 32, 96, 2), ("c", 96, 128, 1)):
        pts = ceremony.decode_points(rows[:, lo:hi].contiguous(), group, compressed=True, checked=True)   # (the index of a column is the proof's)
        out.append(ceremony._no_infinity(pts, f"proof point {name}"))
    return tuple(out)


def write_proofs(a, b, c):
    """the inverse of read_proofs: (n, 8), (n, 16), (n, 8) device records -> a uint8 device tensor of 128 n bytes"""
    import torch

    from . import ceremony

    return torch.cat([ceremony.encode_points(a.contiguous(), True), ceremony.encode_points(b.contiguous(), True),
                      ceremony.encode_points(c.contiguous(), True)], dim=1).reshape(-1)
