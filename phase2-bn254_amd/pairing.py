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
ceremony.g2_subgroup_check establishes it for G2 data from outside.
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
