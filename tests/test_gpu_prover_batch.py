"""prover.create_proofs / circom.prove_many: B witnesses of one circuit over one Parameters, each of the eight multiexps of prover.rs:250-298 as
ONE batched call (bellman.multiexp_many).  The yardstick is create_proof itself -- create_proofs must return, byte for byte, the list of
create_proof's proofs -- and, for proof 0, the proof assembled from the oracle's domain ops, multiexps and group law the way
tests/test_gpu_prover.py assembles it (the instance builder below is that test's, with B witnesses, evaluation vectors and (r, s))."""
import ctypes as C

import numpy as np
import pytest

import bn254_model as M
import golden_util as GU
import inputs
import oracle_lib as O
import r1cs_cases as K

pytestmark = pytest.mark.gpu
R = M.R_ORDER


def _ints(a):
    a = np.asarray(a, dtype=np.uint64).reshape(-1, 4)
    return [int(x[0]) | int(x[1]) << 64 | int(x[2]) << 128 | int(x[3]) << 192 for x in a]


def _limbs(vals):
    return np.array([M.to_limbs(v % R) for v in vals], dtype=np.uint64)


def _mont(vals):
    return _limbs([v * M.MONT_R % R for v in vals])


def _instance(zk, log_m, n_proofs, oracle_data):
    """a synthetic 2^log_m-constraint instance: one Parameters, three densities, n_proofs ProvingAssignments with their own witness-like
    assignments (0 / 1 / uniform), evaluation vectors and (r, s)"""
    import torch

    import bench

    P = zk.prover
    dev = torch.device("cuda", 0)
    L = zk.lib.load()
    m = 1 << log_m
    num_inputs, num_aux = 10, m - 37
    rng = np.random.default_rng(7000 + log_m)

    def synth(group, n, seed):
        k = bench.gen_scalars(n, seed, dev)
        p = torch.empty((n, 8 * group), dtype=torch.int64, device=dev)
        gen = np.ascontiguousarray(inputs.G1_GEN_RAW if group == 1 else inputs.G2_GEN_RAW)
        fn = L.mi355zk_bn254_g1_batch_mul_dev if group == 1 else L.mi355zk_bn254_g2_batch_mul_dev
        assert fn(C.c_void_p(p.data_ptr()), gen.ctypes.data_as(C.c_void_p), C.c_void_p(k.data_ptr()), n, None) == 0
        return p

    def witness(n, seed):
        v = _ints(inputs.random_scalars(n, seed=seed))
        kind = rng.integers(0, 10, size=n)
        return [0 if k < 2 else 1 if k < 5 else x for k, x in zip(kind, v)]

    a_aux_bits = rng.random(num_aux) < 0.5
    b_in_bits = rng.random(num_inputs) < 0.5
    b_aux_bits = rng.random(num_aux) < 0.4
    na, nb_ = int(a_aux_bits.sum()), int(b_in_bits.sum()) + int(b_aux_bits.sum())
    h_b, l_b = synth(1, m - 1, 7120), synth(1, num_aux, 7121)
    a_b, b1_b, b2_b = synth(1, num_inputs + na, 7122), synth(1, nb_, 7123), synth(2, nb_, 7124)
    vk_pts1 = O.G1.mul_many_affine(inputs.G1_GEN_RAW, inputs.random_scalars(3, seed=7130))
    vk_pts2 = O.G2.mul_many_affine(inputs.G2_GEN_RAW, inputs.random_scalars(2, seed=7131))
    vk = {"alpha_g1": vk_pts1[0], "beta_g1": vk_pts1[1], "delta_g1": vk_pts1[2], "beta_g2": vk_pts2[0], "delta_g2": vk_pts2[1]}
    params = P.Parameters(vk, h_b, l_b, a_b, b1_b, b2_b)
    to_dev = lambda arr: torch.from_numpy(np.ascontiguousarray(arr).view(np.int64)).to(dev)  # noqa: E731
    assignments, rs, ss, raw = [], [], [], []
    for i in range(n_proofs):
        inp_c, aux_c = witness(num_inputs, 7200 + 10 * i), witness(num_aux, 7201 + 10 * i)
        inp_c[0] = 1                                                    # the constant ONE input
        if oracle_data and i == 0:
            abc = [_ints(inputs.random_fr_mont(m, seed=7210 + j)) for j in range(3)]
            d_abc = [to_dev(_limbs(v)) for v in abc]
        else:
            abc = None
            d_abc = [to_dev(inputs.random_fr_mont(m, seed=7210 + 10 * i + j)) for j in range(3)]
        # (one DensityTracker object per assignment: create_proofs must compare the words, not the identities)
        assignments.append(P.ProvingAssignment(d_abc[0], d_abc[1], d_abc[2], to_dev(_mont(inp_c)), to_dev(_mont(aux_c)),
                                               zk.DensityTracker.from_bools(a_aux_bits), zk.DensityTracker.from_bools(b_in_bits),
                                               zk.DensityTracker.from_bools(b_aux_bits)))
        rs.append((0x1234567890ABCDEF1122334455667788 + 0x1111 * i) % R)
        ss.append((0x0FEDCBA9876543210F1E2D3C4B5A6978 + 0x7777 * i) % R)
        raw.append((abc, inp_c, aux_c))
    bits = (a_aux_bits, b_in_bits, b_aux_bits)
    return params, assignments, rs, ss, raw, bits


def _oracle_proof(log_m, params, raw0, bits, r, s):
    """the proof of one assignment from the oracle, as tests/test_gpu_prover.py assembles it"""
    m = 1 << log_m
    abc, inp_c, aux_c = raw0
    a_aux_bits, b_in_bits, b_aux_bits = bits
    num_inputs = len(inp_c)
    vk = params.vk
    host = lambda t: t.cpu().numpy().view(np.uint64)  # noqa: E731
    dom = lambda v, op: _ints(O.fr_domain_op(_limbs(v), log_m, op))  # noqa: E731
    ev = [dom(dom(v, "ifft"), "coset_fft") for v in abc]
    rinv = pow(M.MONT_R, -1, R)
    zinv_mont = pow((pow(7, m, R) - 1) % R, -1, R) * M.MONT_R % R
    mmul = lambda x, y: x * y * rinv % R  # noqa: E731
    hq = [mmul((mmul(x, y) - z) % R, zinv_mont) for x, y, z in zip(*ev)]
    hq = dom(hq, "icoset_fft")[:m - 1]
    h_canon = _limbs([v * rinv % R for v in hq])
    inp_l, aux_l = _limbs(inp_c), _limbs(aux_c)

    def mexp(G, bases, off, scalars, b=None):
        rc, out = G.multiexp(host(bases), scalars, density=None if b is None else GU.density_words(b), density_bits=None if b is None else len(b),
                             base_offset=off, threads=8)
        assert rc == 0
        return out

    h_o = mexp(O.G1, params.h, 0, h_canon)
    l_o = mexp(O.G1, params.l, 0, aux_l)
    a_ans = O.G1.add(mexp(O.G1, params.a, 0, inp_l), mexp(O.G1, params.a, num_inputs, aux_l, a_aux_bits))
    nbi = int(b_in_bits.sum())
    b1_ans = O.G1.add(mexp(O.G1, params.b_g1, 0, inp_l, b_in_bits), mexp(O.G1, params.b_g1, nbi, aux_l, b_aux_bits))
    b2_ans = O.G2.add(mexp(O.G2, params.b_g2, 0, inp_l, b_in_bits), mexp(O.G2, params.b_g2, nbi, aux_l, b_aux_bits))
    k = lambda v: np.array(M.to_limbs(v % R), dtype=np.uint64)  # noqa: E731
    g_a = O.G1.add_mixed(O.G1.mul(O.G1.from_affine(vk["delta_g1"]), k(r)), vk["alpha_g1"])
    g_b = O.G2.add_mixed(O.G2.mul(O.G2.from_affine(vk["delta_g2"]), k(s)), vk["beta_g2"])
    g_c = O.G1.mul(O.G1.from_affine(vk["delta_g1"]), k(r * s))
    g_c = O.G1.add(g_c, O.G1.mul(O.G1.from_affine(vk["alpha_g1"]), k(s)))
    g_c = O.G1.add(g_c, O.G1.mul(O.G1.from_affine(vk["beta_g1"]), k(r)))
    g_a = O.G1.add(g_a, a_ans)
    g_c = O.G1.add(g_c, O.G1.mul(a_ans, k(s)))
    g_b = O.G2.add(g_b, b2_ans)
    g_c = O.G1.add(g_c, O.G1.mul(b1_ans, k(r)))
    g_c = O.G1.add(O.G1.add(g_c, h_o), l_o)
    return O.G1.to_affine(g_a), O.G2.to_affine(g_b), O.G1.to_affine(g_c)


def _same(got, want):
    return len(got) == len(want) and all(len(g) == 3 and all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(g, w)) for g, w in zip(got, want))


def test_create_proofs_equals_the_loop_and_the_oracle(zk, worker):
    P = zk.prover
    log_m, n_proofs = 10, 3
    params, assignments, rs, ss, raw, bits = _instance(zk, log_m, n_proofs, oracle_data=True)
    want = [P.create_proof(worker, params, a, r, s) for a, r, s in zip(assignments, rs, ss)]
    assert len({w[2].tobytes() for w in want}) == n_proofs                       # three different proofs
    got = P.create_proofs(worker, params, assignments, rs, ss)
    assert _same(got, want)
    assert _same(P.create_proofs(worker, params, assignments, rs, ss, concurrent=False), want)
    oracle = _oracle_proof(log_m, params, raw[0], bits, rs[0], ss[0])
    assert all(np.array_equal(g, o) for g, o in zip(got[0], oracle))
    # Parameters with window tables: the batch runs over each table's window 0; the same proofs
    tabled = params.with_tables(1, 1)
    assert isinstance(tabled.h, zk.MsmTable) and isinstance(tabled.b_g2, zk.MsmTable)
    assert _same(P.create_proofs(worker, tabled, assignments, rs, ss), want)
    # one proof and no proof
    assert _same(P.create_proofs(worker, params, assignments[:1], rs[:1], ss[:1]), want[:1])
    assert P.create_proofs(worker, params, [], [], []) == []


def test_mismatched_assignments_are_refused(zk, worker):
    P = zk.prover
    params, assignments, rs, ss, _, bits = _instance(zk, 10, 2, oracle_data=False)
    other = np.array(bits[2], copy=True)
    other[5] = not other[5]
    a1 = assignments[1]
    odd = P.ProvingAssignment(a1.a, a1.b, a1.c, a1.input_assignment, a1.aux_assignment, a1.a_aux_density, a1.b_input_density,
                              zk.DensityTracker.from_bools(other))
    with pytest.raises(ValueError):
        P.create_proofs(worker, params, [assignments[0], odd], rs, ss)
    short = P.ProvingAssignment(a1.a, a1.b, a1.c, a1.input_assignment, a1.aux_assignment[:-1], a1.a_aux_density, a1.b_input_density, a1.b_aux_density)
    with pytest.raises(ValueError):
        P.create_proofs(worker, params, [assignments[0], short], rs, ss)
    with pytest.raises(ValueError):
        P.create_proofs(worker, params, assignments, rs[:1], ss)


def test_create_proofs_at_2_to_the_14(zk, worker):
    P = zk.prover
    params, assignments, rs, ss, _, _ = _instance(zk, 14, 4, oracle_data=False)
    want = [P.create_proof(worker, params, a, r, s) for a, r, s in zip(assignments, rs, ss)]
    assert _same(P.create_proofs(worker, params, assignments, rs, ss), want)


def test_prove_many_equals_prove_per_witness(zk, worker):
    """circom.prove_many on the ~200-constraint circuit of tests/test_gpu_r1cs.py, parameters made the way that test makes them"""
    import torch

    r = K.R_ORDER
    circuit = K.random_circuit(zk)
    cs = zk.circom.assemble(circuit)
    m = 1 << zk.circom.domain_exponent(cs.num_constraints)
    tau, alpha, beta = 0x1234567 % r, 0x89ABCDEF01 % r, 0x55AA55AA55 % r
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.int64)).cuda()  # noqa: E731
    limbs = lambda ks: np.stack([np.array(M.to_limbs(k % r), dtype=np.uint64) for k in ks])  # noqa: E731
    mul1 = lambda ks: O.G1.mul_many_affine(inputs.G1_GEN_RAW, limbs(ks))  # noqa: E731
    mul2 = lambda ks: O.G2.mul_many_affine(inputs.G2_GEN_RAW, limbs(ks))  # noqa: E731
    tp = [pow(tau, i, r) for i in range(2 * m - 1)]
    acc = {"hash": torch.zeros(64, dtype=torch.uint8).cuda(), "tau_g1": dev(mul1(tp)), "tau_g2": dev(mul2(tp[:m])),
           "alpha_g1": dev(mul1([alpha * t for t in tp[:m]])), "beta_g1": dev(mul1([beta * t for t in tp[:m]])), "beta_g2": dev(mul2([beta]))}
    radix = zk.ceremony.read_phase1radix2m(zk.ceremony.write_phase1radix2m(zk.ceremony.prepare_phase2(acc, m)), m)
    params = zk.circom.mpc_parameters_new(circuit, False, radix)["params"]
    rng = np.random.default_rng(7400)
    n_vars = circuit.num_inputs + circuit.num_aux
    witnesses = [list(circuit.witness)]
    for _ in range(2):
        kinds = rng.integers(0, 4, size=n_vars)
        witnesses.append([1] + [0 if k == 0 else 1 if k == 1 else int.from_bytes(rng.bytes(40), "little") % r for k in kinds[1:]])
    rs = [(0x1234567890ABCDEF1122334455667788 + i) % r for i in range(3)]
    ss = [(0x0FEDCBA9876543210F1E2D3C4B5A6978 + 5 * i) % r for i in range(3)]
    cc = zk.circom.compile_circuit(circuit, params["h"].device)
    want = []
    for w, rr, s_ in zip(witnesses, rs, ss):
        one = zk.circom.CircomCircuit(circuit.num_inputs, circuit.num_aux, circuit.num_constraints, circuit.constraints, w)
        want.append(zk.circom.prove(worker, one, params, rr, s_, compiled=cc))
    assert len({w[2].tobytes() for w in want}) == 3
    assert _same(zk.circom.prove_many(worker, circuit, params, witnesses, rs, ss, compiled=cc), want)
    assert _same(zk.circom.prove_many(worker, circuit, params, witnesses[:2], rs[:2], ss[:2]), want[:2])   # compiled here
