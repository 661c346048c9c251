"""The pairing kernels (phase2-bn254_amd/csrc/pairing.hip) and the Python layer over them (phase2-bn254_amd/pairing.py) on the device:
golden values byte for byte, the segmented product across every path its lane numbering takes, device against host, same_ratio on what
power_pairs / merge_pairs produce, and groth16 verify_proof on a proof made by this library's own generator and prover.  Expectations come
from tests/pairing_model.py (through tests/golden/pairing_golden.json) -- never from the code under test."""
import ctypes as C
import json
import os
import threading

import numpy as np
import pytest

import bn254_model as M
import inputs
import pairing_model as P

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R = M.R_ORDER
ONE_WORDS = np.array(P.gt_to_words(P.ONE), dtype=np.uint64)


def dev(a):
    import torch

    a = np.ascontiguousarray(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def host(t):
    return t.cpu().numpy().view(np.uint64)


def limbs(values):
    return np.array([M.to_limbs(v % R) for v in values], dtype=np.uint64).reshape(-1, 4)


def ints(limb_rows):
    return [M.from_limbs(row) for row in limb_rows]


def batch_mul(zk, group, scalars):
    """scalars[i] * generator on the device (mi355zk_bn254_g{1,2}_batch_mul_dev): (n, 8 * group) int64 device records"""
    import torch

    lib = zk.lib.load()
    k = dev(limbs(scalars))
    out = torch.empty((k.shape[0], 8 * group), dtype=torch.int64, device="cuda")
    gen = inputs.G1_GEN_RAW if group == 1 else inputs.G2_GEN_RAW
    fn = lib.mi355zk_bn254_g1_batch_mul_dev if group == 1 else lib.mi355zk_bn254_g2_batch_mul_dev
    assert fn(C.c_void_p(out.data_ptr()), gen.ctypes.data_as(C.c_void_p), C.c_void_p(k.data_ptr()), k.shape[0], None) == 0
    torch.cuda.synchronize()
    return out


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(ROOT, "tests", "golden", "pairing_golden.json")) as f:
        g = json.load(f)
    words = lambda h: np.array([int(x, 16) for x in h], dtype=np.uint64)  # noqa: E731
    raw1 = lambda p: np.array(M.g1_affine_to_raw(p), dtype=np.uint64)  # noqa: E731
    raw2 = lambda p: np.array(M.g2_affine_to_raw(p), dtype=np.uint64)  # noqa: E731
    g1, g2, gt = [inputs.G1_GEN_RAW], [inputs.G2_GEN_RAW], [words(g["e_g1_g2"])]
    for e in g["pairs"]:
        g1.append(raw1(M.ec_mul(M.FQ_OPS, M.G1_GEN, int(e["a"], 16))))
        g2.append(raw2(M.ec_mul(M.FQ2_OPS, M.G2_GEN, int(e["b"], 16))))
        gt.append(words(e["gt"]))
    for e in g["jeff1"]:
        g1.append(words(e["g1"]))
        g2.append(words(e["g2"]))
        gt.append(words(e["gt"]))
    return {"g1": np.stack(g1), "g2": np.stack(g2), "gt": np.stack(gt), "e": P.gt_from_words(words(g["e_g1_g2"]))}


def gt_power(golden, k):
    """e(G1, G2)^k in the 384-byte format, by the model"""
    return np.array(P.gt_to_words(P.f12_pow(golden["e"], k % R)), dtype=np.uint64)


def test_golden_pairs_byte_for_byte(zk, worker, golden):
    import torch

    g1, g2 = dev(golden["g1"]), dev(golden["g2"])
    n = g1.shape[0]
    assert n == 9
    got = zk.pairing.pairing_product(g1, g2)
    assert np.array_equal(host(got), golden["gt"])
    ptr = torch.arange(0, n + 1, dtype=torch.int32, device="cuda")
    assert np.array_equal(host(zk.pairing.pairing_product(g1, g2, ptr)), golden["gt"])
    # the two jeff1 pairs as one group: one (EIP-197), and the comparison kernels on these values
    ptr = torch.tensor([0, 7, 9], dtype=torch.int32, device="cuda")
    grouped = zk.pairing.pairing_product(g1, g2, ptr)
    assert np.array_equal(host(grouped)[1], ONE_WORDS)
    assert zk.pairing.gt_eq(grouped).cpu().tolist() == [False, True]
    assert zk.pairing.gt_eq(got, dev(np.roll(golden["gt"], 1, axis=0))).cpu().tolist() == [False] * n
    assert zk.pairing.gt_eq(got, dev(golden["gt"])).cpu().tolist() == [True] * n


GROUP_LENGTHS = (0, 1, 2, 3, 63, 64, 65, 129, 1025)


def test_segmented_product_across_run_and_pass_boundaries(zk, worker, golden):
    """group lengths across the wave width, the 64-value run and a second product pass, in ONE call: every group is
    e(G1, G2)^(sum a_i b_i mod r); then the same call with a zero P and a zero Q planted in the 65-group, whose terms drop out"""
    total = sum(GROUP_LENGTHS)
    a, b = ints(inputs.random_scalars(total, seed=901)), ints(inputs.random_scalars(total, seed=902))
    a[5], b[5] = R - 1, R - 1
    g1, g2 = batch_mul(zk, 1, a), batch_mul(zk, 2, b)
    ptr = np.concatenate([[0], np.cumsum(GROUP_LENGTHS)]).astype(np.int32)
    got = host(zk.pairing.pairing_product(g1, g2, dev(ptr)))
    assert got.shape == (len(GROUP_LENGTHS), 48)
    for g, length in enumerate(GROUP_LENGTHS):
        lo, hi = int(ptr[g]), int(ptr[g + 1])
        want = gt_power(golden, sum(x * y for x, y in zip(a[lo:hi], b[lo:hi])))
        assert np.array_equal(got[g], want), length
    assert np.array_equal(got[0], ONE_WORDS)                 # the empty group
    lo = int(ptr[GROUP_LENGTHS.index(65)])
    zp, zq = lo + 17, lo + 64                                 # inside the first run of the group, and alone in its second run
    g1[zp] = 0
    g2[zq] = 0
    got2 = host(zk.pairing.pairing_product(g1, g2, dev(ptr)))
    keep = [i for i in range(lo, lo + 65) if i not in (zp, zq)]
    for g in range(len(GROUP_LENGTHS)):
        want = gt_power(golden, sum(a[i] * b[i] for i in keep)) if GROUP_LENGTHS[g] == 65 else got[g]
        assert np.array_equal(got2[g], want), GROUP_LENGTHS[g]


def test_device_matches_host_and_two_streams_agree(zk, worker):
    import torch

    lib = zk.lib.load()
    n = 64
    g1 = batch_mul(zk, 1, ints(inputs.random_scalars(n, seed=911)))
    g2 = batch_mul(zk, 2, ints(inputs.random_scalars(n, seed=912)))
    got = host(zk.pairing.pairing_product(g1, g2))
    h1, h2 = np.ascontiguousarray(host(g1)), np.ascontiguousarray(host(g2))
    for i in range(n):
        out = np.zeros(48, dtype=np.uint64)
        assert lib.mi355zk_bn254_pairing_product(out.ctypes.data_as(C.c_void_p), h1[i].ctypes.data_as(C.c_void_p), h2[i].ctypes.data_as(C.c_void_p), 1) == 0
        assert np.array_equal(got[i], out), i
    # the whole vector as one group, host against device
    out = np.zeros(48, dtype=np.uint64)
    assert lib.mi355zk_bn254_pairing_product(out.ctypes.data_as(C.c_void_p), h1.ctypes.data_as(C.c_void_p), h2.ctypes.data_as(C.c_void_p), n) == 0
    assert np.array_equal(host(zk.pairing.pairing_product(g1, g2, dev(np.array([0, n], dtype=np.int32))))[0], out)
    torch.cuda.synchronize()
    results = [None, None]

    def call(k):
        with torch.cuda.stream(torch.cuda.Stream()):
            r = zk.pairing.pairing_product(g1, g2)
            torch.cuda.current_stream().synchronize()
            results[k] = host(r)

    threads = [threading.Thread(target=call, args=(k,)) for k in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert np.array_equal(results[0], got) and np.array_equal(results[1], got)


def test_same_ratio(zk, worker):
    import torch

    x, s, t = 0x1F3C5A7E9B2D4F60718293A4B5C6D7E8F9 % R, 0x5DEECE66D, R - 12345
    g1 = batch_mul(zk, 1, [s, s * x])
    g2 = batch_mul(zk, 2, [t, t * x, t * (x + 1)])
    assert zk.pairing.same_ratio((g1[0], g1[1]), (g2[0], g2[1]))                      # device tensors: the kernels
    assert not zk.pairing.same_ratio((g1[0], g1[1]), (g2[0], g2[2]))
    h1, h2 = host(g1), host(g2)
    assert zk.pairing.same_ratio((h1[0], h1[1]), (h2[0], h2[1]))                      # host records: the host product
    for pos in range(4):
        pts = [g1[0], g1[1], g2[0], g2[1]]
        pts[pos] = torch.zeros_like(pts[pos])
        assert not zk.pairing.same_ratio((pts[0], pts[1]), (pts[2], pts[3])), pos
    # 65 checks, the false one at each place in turn (both sides of the wave width)
    n = 65
    xs, ss, ts = (ints(inputs.random_scalars(n, seed=k)) for k in (921, 922, 923))
    g1_a, g1_b = batch_mul(zk, 1, ss), batch_mul(zk, 1, [a * b for a, b in zip(ss, xs)])
    g2_a, g2_b = batch_mul(zk, 2, ts), batch_mul(zk, 2, [a * b for a, b in zip(ts, xs)])
    assert zk.pairing.same_ratio_batch(g1_a, g1_b, g2_a, g2_b).tolist() == [True] * n
    for bad in (0, 31, 63, 64):
        wrong = g2_b.clone()
        wrong[bad] = g2_b[(bad + 1) % n]
        assert zk.pairing.same_ratio_batch(g1_a, g1_b, g2_a, wrong).tolist() == [i != bad for i in range(n)], bad
    zeroed = g1_b.clone()
    zeroed[7] = 0
    assert zk.pairing.same_ratio_batch(g1_a, zeroed, g2_a, g2_b).tolist() == [i != 7 for i in range(n)]


def test_same_ratio_of_power_pairs_and_merge_pairs(zk, worker):
    """utils.rs:90-109 with the pairing in place of the secret: same_ratio(power_pairs(tau table), (g2, tau g2)) on a 2^8 table, the same
    for the G2 table against (g1, tau g1), and merge_pairs of the table with its alpha multiple against (g2, alpha g2)"""
    to_affine = zk.prover._to_affine
    tau, alpha = 0x2F0E1D2C3B4A59687796A5B4C3D2E1F00F1E2D3C4B5A69788796A5B4C3D2E1F % R, 0x1B7E4D3C2A190807F6E5D4C3B2A1908F % R
    n = 1 << 8
    powers = [pow(tau, i, R) for i in range(n)]
    tau_g1, tau_g2 = batch_mul(zk, 1, powers), batch_mul(zk, 2, powers)
    alpha_tau_g1 = batch_mul(zk, 1, [alpha * p for p in powers])
    g1_pair, g2_pair, g2_alpha = host(tau_g1[:2]), host(tau_g2[:2]), host(batch_mul(zk, 2, [1, alpha]))
    rho = dev(inputs.random_scalars(n - 1, seed=931))
    s, sx = zk.ceremony.power_pairs(tau_g1, rho)
    assert zk.pairing.same_ratio((to_affine(s), to_affine(sx)), (g2_pair[0], g2_pair[1]))
    s2, sx2 = zk.ceremony.power_pairs(tau_g2, rho)
    assert zk.pairing.same_ratio((g1_pair[0], g1_pair[1]), (to_affine(s2), to_affine(sx2)))
    rho_n = dev(inputs.random_scalars(n, seed=932))
    m, mx = zk.ceremony.merge_pairs(tau_g1, alpha_tau_g1, rho_n)
    assert zk.pairing.same_ratio((to_affine(m), to_affine(mx)), (g2_alpha[0], g2_alpha[1]))
    assert not zk.pairing.same_ratio((to_affine(m), to_affine(mx)), (g2_pair[0], g2_pair[1]))
    tampered = tau_g1.clone()
    tampered[1] = tau_g1[2]                                  # utils.rs:106: one wrong power
    s3, sx3 = zk.ceremony.power_pairs(tampered, rho)
    assert not zk.pairing.same_ratio((to_affine(s3), to_affine(sx3)), (g2_pair[0], g2_pair[1]))


# fixed non-zero toxic waste and proof randomness
ALPHA, BETA, GAMMA, DELTA, TAU = (0x1B7E4D3C2A190807F6E5D4C3B2A1908F7E6D5C4B3A29180706F5E4D3C2B1A09 % R, 0x2468ACE013579BDF02468ACE13579BDF2468ACE013579BDF02468ACE13579BD % R,
                                  0x0123456789ABCDEF0FEDCBA9876543210123456789ABCDEF0FEDCBA98765432 % R, R - 0x5DEECE66D, 0x2F0E1D2C3B4A59687796A5B4C3D2E1F00F1E2D3C4B5A69788796A5B4C3D2E1F % R)


def chain_circuit(zk, steps=4, c=7, x0=3):
    """x_{i+1} = x_i * x_i + c: variable 0 is ONE, 1 the public output x_steps, the aux variables x_0 .. x_{steps-1}"""
    xs = [x0]
    for _ in range(steps):
        xs.append((xs[-1] * xs[-1] + c) % R)
    var = lambda i: 1 if i == steps else 2 + i  # noqa: E731
    constraints = [([(var(i), 1)], [(var(i), 1)], [(var(i + 1), 1), (0, R - c)]) for i in range(steps)]
    witness = [1, xs[steps]] + xs[:steps]
    for a, b, cc in constraints:
        ev = lambda lc: sum(k * witness[v] for v, k in lc) % R  # noqa: E731
        assert ev(a) * ev(b) % R == ev(cc)
    return zk.circom.CircomCircuit(2, steps, steps, constraints, witness)


def test_verify_proof(zk, worker):
    circuit = chain_circuit(zk)
    params = zk.generator.generate_parameters(circuit, inputs.G1_GEN_RAW, inputs.G2_GEN_RAW, ALPHA, BETA, GAMMA, DELTA, TAU, "cuda")
    r, s = 0x3C4B5A69788796A5B4C3D2E1F00F1E2D % R, 0x1F2E3D4C5B6A79880796A5B4C3D2E1F0 % R
    a, b, c = (np.asarray(p, dtype=np.uint64).reshape(-1) for p in zk.circom.prove(worker, circuit, params, r, s))
    pvk = zk.pairing.prepare_verifying_key(params["vk"])
    public = [circuit.witness[1]]
    assert pvk["ic"].shape[0] == 2
    assert zk.pairing.verify_proof(pvk, (a, b, c), public) is True
    assert zk.pairing.verify_proof(pvk, (a, b, c), [public[0] + 1]) is False
    two_c = zk.prover._to_affine(zk.prover._mul(c, 2))
    assert zk.pairing.verify_proof(pvk, (a, b, two_c), public) is False
    assert zk.pairing.verify_proof(pvk, (c, b, a), public) is False
    with pytest.raises(zk.SynthesisError) as e:
        zk.pairing.verify_proof(pvk, (a, b, c), public + [1])
    assert e.value.kind == zk.SynthesisError.MALFORMED_VERIFYING_KEY
    # 33 proofs in one launch: the honest one repeated, a bad one at both ends and in the middle
    proofs, pubs = [(a, b, c)] * 33, [public] * 33
    proofs[0], proofs[32] = (a, b, two_c), (c, b, a)
    pubs[16] = [public[0] + 1]
    assert zk.pairing.verify_proofs(pvk, proofs, pubs).tolist() == [i not in (0, 16, 32) for i in range(33)]


def test_empty_calls_and_bad_arguments(zk, worker, golden):
    import torch

    lib = zk.lib.load()
    assert lib.mi355zk_bn254_pairing_product_dev(None, None, None, 0, None, 0, None) == 0
    assert lib.mi355zk_bn254_gt_is_one_dev(None, None, 0, None) == 0 and lib.mi355zk_bn254_gt_eq_dev(None, None, None, 0, None) == 0
    empty = zk.pairing.pairing_product(torch.empty((0, 8), dtype=torch.int64, device="cuda"), torch.empty((0, 16), dtype=torch.int64, device="cuda"))
    assert tuple(empty.shape) == (0, 48)
    g1, g2 = dev(golden["g1"]), dev(golden["g2"])
    out = torch.zeros((9, 48), dtype=torch.int64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    bad = zk.lib.ERR_BAD_ARGS
    assert lib.mi355zk_bn254_pairing_product_dev(None, p(g1), p(g2), 9, None, 9, None) == bad
    assert lib.mi355zk_bn254_pairing_product_dev(p(out), None, p(g2), 9, None, 9, None) == bad
    assert lib.mi355zk_bn254_pairing_product_dev(p(out), p(g1), None, 9, None, 9, None) == bad
    assert lib.mi355zk_bn254_pairing_product_dev(p(out), p(g1), p(g2), 9, None, 8, None) == bad      # no group_ptr: one group per pair
    assert lib.mi355zk_bn254_pairing_product_dev(p(out), p(g1), p(g2), 1 << 31, None, 1 << 31, None) == bad
    assert lib.mi355zk_bn254_gt_is_one_dev(None, p(out), 9, None) == bad and lib.mi355zk_bn254_gt_eq_dev(p(out), p(out), None, 9, None) == bad
    torch.cuda.synchronize()
    assert not host(out).any()                               # nothing was launched
    # groups without pairs: three empty groups give three ones
    ptr = torch.zeros(4, dtype=torch.int32, device="cuda")
    ones = zk.pairing.pairing_product(g1[:0], g2[:0], ptr)
    assert np.array_equal(host(ones), np.tile(ONE_WORDS, (3, 1)))
