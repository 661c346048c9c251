"""Powers-of-tau files streamed through the device (phase2-bn254_amd/stream.py over mi355zk_bn254_g{1,2}_accumulator_transform /
_accumulator_power_pairs) against the in-memory flows of verify.py on the same bytes: a power-4 accumulator (tau_g1: 31, tau_g2 / alpha_g1 /
beta_g1: 16, beta_g2: 1), cut by batch sizes and device pieces that put chunk and piece boundaries everywhere, the real piece size once."""
import ctypes as C

import numpy as np
import pytest

import bn254_model as M
import ceremony_model as CM
import inputs
import oracle_lib as O

pytestmark = pytest.mark.gpu

POWER = 4
KEY = bytes(range(32))
CUTS = [(2, 0), (5, 0), (16, 3), (1000, 0)]                       # (batch_size, piece)
SECRETS1 = (0xABCDEF123456789, 0x1111222233334444, 0x9999AAAABBBB)
SECRETS2 = (0x1F3C5A7E9B2D4F607, 0x718293A4B5C6D7E8, 0x13579BDF02468ACE)
VECTORS = ("tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2")


def _np(t) -> np.ndarray:
    return t.cpu().numpy()


def _dev(a):
    import torch

    a = np.array(a)                                               # (a writable copy: frombuffer views of bytes are not)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def _limbs(v):
    return np.array(M.to_limbs(v % M.R_ORDER), dtype=np.uint64)


@pytest.fixture(scope="module")
def chain(zk, worker, tmp_path_factory):
    """challenge 0 -> response 1 -> challenge 1 -> response 2 from the in-memory flows, as bytes and as files"""
    import torch

    d = tmp_path_factory.mktemp("chain")
    out = {"dir": d}
    out["challenge0"] = _np(zk.ceremony.write_accumulator(zk.ceremony.new_accumulator(POWER, torch.device("cuda", 0)), compressed=False)).tobytes()
    r1, out["pub1"] = zk.contribute_response(out["challenge0"], POWER, *SECRETS1)
    out["response1"] = _np(r1).tobytes()
    out["challenge1"] = _np(zk.next_challenge(r1, POWER)).tobytes()
    r2, out["pub2"] = zk.contribute_response(out["challenge1"], POWER, *SECRETS2)
    out["response2"] = _np(r2).tobytes()
    for name in ("challenge0", "response1", "challenge1", "response2"):
        (d / name).write_bytes(out[name])
    out["body"] = zk.ceremony.accumulator_layout(POWER, True)[1]
    return out


@pytest.fixture
def launches(zk, monkeypatch):
    """counts the pairing launches (pairing.pairing_product) of the test, as tests/test_gpu_verify.py does"""
    calls = []
    real = zk.pairing.pairing_product

    def counted(*args, **kwargs):
        calls.append(int(args[0].shape[0]))
        return real(*args, **kwargs)

    monkeypatch.setattr(zk.pairing, "pairing_product", counted)
    return calls


def test_new_constrained_is_the_in_memory_challenge(zk, worker, chain, tmp_path):
    digest = zk.new_constrained(tmp_path / "challenge", POWER, 5)
    assert (tmp_path / "challenge").read_bytes() == chain["challenge0"]
    assert digest == zk.ceremony.calculate_hash(np.frombuffer(chain["challenge0"], dtype=np.uint8))


@pytest.mark.parametrize("batch_size,piece", CUTS)
def test_streamed_contribution_is_the_in_memory_response(zk, worker, chain, tmp_path, batch_size, piece):
    path = tmp_path / "response"
    pub, digest = zk.compute_constrained(chain["dir"] / "challenge0", path, POWER, batch_size, *SECRETS1, piece=piece)
    got = path.read_bytes()
    body = chain["body"]
    assert len(got) == body + zk.keys.PUBLIC_KEY_SIZE and digest == zk.calculate_hash_file(path)
    assert got[:body] == chain["response1"][:body]                   # (the public key holds fresh randomness)
    assert got[:64] == zk.ceremony.calculate_hash(np.frombuffer(chain["challenge0"], dtype=np.uint8))
    assert got[body:] == zk.keys.write_public_key(pub)
    after, pub_read = zk.verify.read_response(got, POWER)
    want = O.G1.mul_many_affine(inputs.G1_GEN_RAW, np.stack([_limbs(pow(SECRETS1[0], i, M.R_ORDER)) for i in (1, 14)]))
    assert np.array_equal(_np(after["tau_g1"][[1, 14]]).view(np.uint64), want)
    before = zk.ceremony.read_accumulator(_dev(np.frombuffer(chain["challenge0"], dtype=np.uint8)), POWER, compressed=False)
    assert zk.verify_transform(before, after, pub_read, got[:64], key=KEY) is True


def _power_pairs(zk, b, data: np.ndarray, key, stream_id, out: np.ndarray = None, piece=0, check_subgroup=1, n=None):
    """one accumulator_power_pairs call over chunk `b` of a compressed body `data` -> (rc, index, s, sx)"""
    L = zk.lib.load()
    s, sx = np.zeros(12 * b.group, np.uint64), np.zeros(12 * b.group, np.uint64)
    idx = C.c_longlong(-7)
    rc = getattr(L, f"mi355zk_bn254_g{b.group}_accumulator_power_pairs")(
        C.c_void_p(data.ctypes.data + b.compressed_offset), b.verify_count if n is None else n, 1, 1, check_subgroup, zk.ceremony._chacha_key(key),
        stream_id, b.start, C.c_void_p(out.ctypes.data + b.uncompressed_offset) if out is not None and b.count else None, piece,
        s.ctypes.data_as(C.c_void_p), sx.ctypes.data_as(C.c_void_p), C.byref(idx))
    return rc, idx.value, s, sx


@pytest.fixture(scope="module")
def whole_sums(zk, worker, chain):
    """power_pairs_random of each decoded whole vector of response 1 under (KEY, the vector's number), as affine records"""
    after, _ = zk.verify.read_response(chain["response1"], POWER)
    to_affine = zk.prover._to_affine
    out = {}
    for sid, name in enumerate(VECTORS[:4]):
        s, sx = zk.ceremony.power_pairs_random(after[name].contiguous(), KEY, sid)
        out[name] = (to_affine(s), to_affine(sx))
    return out


@pytest.mark.parametrize("batch_size,piece", CUTS)
def test_chunked_power_pairs_sums_are_the_whole_vectors(zk, worker, chain, whole_sums, batch_size, piece):
    data = np.frombuffer(chain["response1"], dtype=np.uint8).copy()
    new = np.zeros(len(chain["challenge1"]), dtype=np.uint8)
    add, to_affine = zk.prover._add, zk.prover._to_affine
    sums = {}
    for b in zk.batches(POWER, batch_size):
        rc, idx, s, sx = _power_pairs(zk, b, data, KEY, VECTORS.index(b.vector), new, piece)
        assert (rc, idx) == (0, -1), (b, rc, idx)
        sums[b.vector] = (s, sx) if b.vector not in sums else (add(sums[b.vector][0], s), add(sums[b.vector][1], sx))
    for name in VECTORS[:4]:
        assert np.array_equal(to_affine(sums[name][0]), whole_sums[name][0]), name
        assert np.array_equal(to_affine(sums[name][1]), whole_sums[name][1]), name
    assert not to_affine(sums["beta_g2"][0]).any() and not to_affine(sums["beta_g2"][1]).any()      # one element: no pair
    assert new[64:].tobytes() == chain["challenge1"][64:]          # the records re-encoded uncompressed: next_challenge's body, for every cut


@pytest.mark.parametrize("batch_size,piece", CUTS)
def test_streamed_verification_accepts_a_chain_of_two_contributions(zk, worker, chain, tmp_path, launches, batch_size, piece):
    d = chain["dir"]
    # in-memory files in both roles
    got = zk.verify_transform_constrained(d / "challenge0", d / "response1", tmp_path / "c1", POWER, batch_size, piece=piece)
    assert launches == [22]                                          # eleven same_ratio checks, ONE launch
    assert (tmp_path / "c1").read_bytes() == chain["challenge1"]
    assert got == (zk.calculate_hash_file(d / "response1"), zk.calculate_hash_file(tmp_path / "c1"))
    assert got[0] == chain["challenge1"][:64]
    zk.verify_transform_constrained(d / "challenge1", d / "response2", tmp_path / "c2", POWER, batch_size, key=KEY, piece=piece)
    assert (tmp_path / "c2").read_bytes() == _np(zk.next_challenge(chain["response2"], POWER)).tobytes()
    # streamed files in both roles: a contribution to the streamed new challenge, verified against it; and the in-memory flow accepts it
    zk.compute_constrained(tmp_path / "c1", tmp_path / "r2", POWER, batch_size, piece=piece)
    n = len(launches)
    zk.verify_transform_constrained(tmp_path / "c1", tmp_path / "r2", tmp_path / "c2s", POWER, batch_size, piece=piece)
    assert launches[n:] == [22]
    r2 = (tmp_path / "r2").read_bytes()
    assert (tmp_path / "c2s").read_bytes() == _np(zk.next_challenge(r2, POWER)).tobytes()
    before = zk.ceremony.read_accumulator(_dev(np.frombuffer(chain["challenge1"], dtype=np.uint8)), POWER, compressed=False)
    after, pub = zk.verify.read_response(r2, POWER)
    assert zk.verify_transform(before, after, pub, zk.ceremony.calculate_hash(np.frombuffer(chain["challenge1"], dtype=np.uint8))) is True
    # the second response does not verify against the first challenge: its head is another file's hash
    with pytest.raises(zk.VerificationError) as e:
        zk.verify_transform_constrained(d / "challenge0", d / "response2", tmp_path / "c3", POWER, batch_size, piece=piece)
    assert e.value.check == "challenge hash" and not (tmp_path / "c3").exists()


@pytest.fixture(scope="module")
def transform1(zk, worker, chain):
    before = zk.ceremony.read_accumulator(_dev(np.frombuffer(chain["challenge0"], dtype=np.uint8)), POWER, compressed=False)
    after, pub = zk.verify.read_response(chain["response1"], POWER)
    return before, after, pub, chain["response1"][:64]


def _rebuilt(zk, chain, acc) -> bytes:
    """response 1 with the accumulator `acc` in place of its own"""
    return _np(zk.ceremony.write_accumulator(acc, compressed=True)).tobytes() + chain["response1"][chain["body"]:]


@pytest.mark.parametrize("vector,indices", [("tau_g1", (4, 5, 15, 16, 30)), ("tau_g2", (0, 8, 15)), ("alpha_g1", (0, 8, 15)), ("beta_g1", (0, 8, 15)),
                                            ("beta_g2", (0,))])
def test_one_scaled_element_at_the_cuts_is_rejected_as_in_memory(zk, worker, chain, transform1, tmp_path, launches, vector, indices):
    """batch_size 5: chunk boundaries at 4 | 5 and at the junction 15 | 16 of the two ranges of tau_g1"""
    before, after, pub, digest = transform1
    for idx in indices:
        bad = dict(after)
        bad[vector] = after[vector].clone()
        k = _dev(_limbs(0x1234567 + idx).reshape(1, 4))
        bad[vector][idx] = zk.ceremony.batch_exp(bad[vector][idx].reshape(1, -1).contiguous(), k, same_scalar=True).reshape(-1)
        with pytest.raises(zk.VerificationError) as want:
            zk.verify_transform(before, bad, pub, digest, key=KEY)
        (tmp_path / "bad").write_bytes(_rebuilt(zk, chain, bad))
        n = len(launches)
        with pytest.raises(zk.VerificationError) as got:
            zk.verify_transform_constrained(chain["dir"] / "challenge0", tmp_path / "bad", tmp_path / "new", POWER, 5, key=KEY)
        assert got.value.check == want.value.check, (vector, idx)
        assert launches[n:] == [22] and not (tmp_path / "new").exists()


def _with_record(data: bytes, offset: int, record: bytes) -> bytes:
    return data[:offset] + record + data[offset + len(record):]


def _g1_x_off_the_curve() -> int:
    """the first x with x^3 + 3 a non-residue: no point of G1 has it"""
    for x in range(1, 100):
        if pow((x * x * x + 3) % M.Q, (M.Q - 1) // 2, M.Q) != 1:
            return x
    raise AssertionError("no x found")


@pytest.mark.parametrize("record,kind", [(M.Q.to_bytes(32, "big"), "CoordinateDecodingError"), (_g1_x_off_the_curve().to_bytes(32, "big"), "NotOnCurve")],
                         ids=["coordinate", "curve"])
def test_a_bad_record_in_the_second_chunk_is_reported_with_its_global_index(zk, worker, chain, tmp_path, record, kind):
    layout = {name: off for name, _, _, off in zk.ceremony.accumulator_layout(POWER, True)[0]}
    for vector, idx in (("alpha_g1", 7), ("tau_g1", 21)):
        bad = _with_record(chain["response1"], layout[vector] + 32 * idx, record)
        with pytest.raises(zk.ceremony.GroupDecodingError) as want:
            zk.verify.read_response(bad, POWER)
        assert (want.value.kind, want.value.index) == (kind, idx)
        (tmp_path / "bad").write_bytes(bad)
        with pytest.raises(zk.ceremony.GroupDecodingError) as got:
            zk.verify_transform_constrained(chain["dir"] / "challenge0", tmp_path / "bad", tmp_path / "new", POWER, 5, piece=3)
        assert (got.value.kind, got.value.index) == (kind, idx)
        assert not (tmp_path / "new").exists()


def test_an_infinity_record_in_the_challenge_is_a_deserialization_error(zk, worker, chain, tmp_path):
    layout = {name: off for name, _, _, off in zk.ceremony.accumulator_layout(POWER, False)[0]}
    for vector, size, idx in (("tau_g1", 64, 6), ("tau_g2", 128, 9)):
        bad = _with_record(chain["challenge0"], layout[vector] + size * idx, bytes([0x40]) + bytes(size - 1))
        with pytest.raises(zk.ceremony.DeserializationError):
            zk.contribute_response(bad, POWER, *SECRETS1)
        (tmp_path / "bad").write_bytes(bad)
        with pytest.raises(zk.ceremony.DeserializationError):
            zk.compute_constrained(tmp_path / "bad", tmp_path / "response", POWER, 5, *SECRETS1, piece=4)
        assert not (tmp_path / "response").exists()
    # the same record in a response: the index is that of the whole vector
    layout = {name: off for name, _, _, off in zk.ceremony.accumulator_layout(POWER, True)[0]}
    data = np.frombuffer(_with_record(chain["response1"], layout["tau_g1"] + 32 * 6, bytes([0x40]) + bytes(31)), dtype=np.uint8).copy()
    b = [b for b in zk.batches(POWER, 5) if b.vector == "tau_g1" and b.start == 5][0]
    rc, idx, _, _ = _power_pairs(zk, b, data, KEY, 0, piece=0)
    assert (rc, idx) == (zk.lib.ERR_POINT_AT_INFINITY, 1)


def _off_subgroup_g2() -> np.ndarray:
    """a point of the twist outside the order-r subgroup, as tests/test_gpu_verify.py makes one"""
    for c in range(1, 50):
        x = (c, 0)
        y = CM.f2_sqrt(M.f2_add(M.f2_mul(M.f2_mul(x, x), x), M.B_G2))
        if y is not None and M.ec_mul(M.FQ2_OPS, (x, y), M.R_ORDER) is not None:
            return np.array(M.g2_affine_to_raw((x, y)), dtype=np.uint64)
    raise AssertionError("no point found")


def test_a_tau_g2_record_outside_the_subgroup_is_rejected(zk, worker, chain, transform1, tmp_path, launches):
    before, after, pub, digest = transform1
    bad = dict(after)
    bad["tau_g2"] = after["tau_g2"].clone()
    bad["tau_g2"][11] = _dev(_off_subgroup_g2())
    with pytest.raises(zk.VerificationError) as want:
        zk.verify_transform(before, bad, pub, digest)
    assert want.value.check == "g2 subgroup"
    (tmp_path / "bad").write_bytes(_rebuilt(zk, chain, bad))
    with pytest.raises(zk.VerificationError) as got:
        zk.verify_transform_constrained(chain["dir"] / "challenge0", tmp_path / "bad", tmp_path / "new", POWER, 5)
    assert got.value.check == "g2 subgroup" and launches == [] and not (tmp_path / "new").exists()
    # the C entry point names the record: code 5 (NotInSubgroup), index within the call
    data = np.frombuffer((tmp_path / "bad").read_bytes(), dtype=np.uint8).copy()
    b = [b for b in zk.batches(POWER, 5) if b.vector == "tau_g2" and b.start == 10][0]
    assert _power_pairs(zk, b, data, KEY, 1)[:2] == (5, 1)
    assert _power_pairs(zk, b, data, KEY, 1, check_subgroup=0)[:2] == (0, -1)
    try:                                                             # the reference's behaviour: unspecified verdict, no fault
        zk.verify_transform_constrained(chain["dir"] / "challenge0", tmp_path / "bad", tmp_path / "new", POWER, 5, check_g2_subgroup=False)
    except zk.VerificationError as e:
        assert e.check != "g2 subgroup"


def test_argument_checks(zk, worker, chain, tmp_path, monkeypatch, launches):
    d = chain["dir"]
    # a response that is not headed by its challenge's hash: rejected before any device call
    def no_device(*args, **kwargs):
        raise AssertionError("a device call was made")

    with monkeypatch.context() as m:
        m.setattr(zk.stream, "_run", no_device)
        m.setattr(zk.ceremony, "g2_subgroup_check", no_device)
        head = bytearray(chain["response1"])
        head[17] ^= 1
        (tmp_path / "bad").write_bytes(bytes(head))
        with pytest.raises(zk.VerificationError) as e:
            zk.verify_transform_constrained(d / "challenge0", tmp_path / "bad", tmp_path / "new", POWER, 5)
        assert e.value.check == "challenge hash" and launches == [] and not (tmp_path / "new").exists()
        # wrong file sizes
        (tmp_path / "short").write_bytes(chain["challenge0"][:-1])
        (tmp_path / "long").write_bytes(chain["response1"] + b"\0")
        with pytest.raises(ValueError):
            zk.compute_constrained(tmp_path / "short", tmp_path / "response", POWER, 5)
        with pytest.raises(ValueError):
            zk.compute_constrained(d / "challenge0", tmp_path / "response", POWER + 1, 5)
        with pytest.raises(ValueError):
            zk.verify_transform_constrained(tmp_path / "short", d / "response1", tmp_path / "new", POWER, 5)
        with pytest.raises(ValueError):
            zk.verify_transform_constrained(d / "challenge0", tmp_path / "long", tmp_path / "new", POWER, 5)
        with pytest.raises(ValueError):
            zk.compute_constrained(d / "challenge0", tmp_path / "response", POWER, 1)
        assert not (tmp_path / "response").exists() and not (tmp_path / "new").exists()
    # the C entry points: null pointers, n >= 2^31, a piece of one point
    L = zk.lib.load()
    buf, out = np.zeros(4 * 128, np.uint8), np.zeros(4 * 128, np.uint8)
    s, sx = np.zeros(24, np.uint64), np.zeros(24, np.uint64)
    tau = (C.c_uint64 * 4)(5, 0, 0, 0)
    too_big = (C.c_uint64 * 4)(*[(1 << 64) - 1] * 4)                 # not a canonical FrRepr
    p = lambda a: a.ctypes.data_as(C.c_void_p)  # noqa: E731
    key = zk.ceremony._chacha_key(KEY)
    idx = C.c_longlong(0)
    for g in (1, 2):
        tr = getattr(L, f"mi355zk_bn254_g{g}_accumulator_transform")
        pp = getattr(L, f"mi355zk_bn254_g{g}_accumulator_power_pairs")
        for args in ((None, p(buf), 4, 0, tau, None, 0, 1, 0, 0, 0), (p(out), None, 4, 0, tau, None, 0, 1, 0, 0, 0), (p(out), p(buf), 4, 0, None, None, 0, 1, 0, 0, 0),
                     (p(out), p(buf), 1 << 31, 0, tau, None, 0, 1, 0, 0, 0), (p(out), p(buf), 4, 0, tau, None, 0, 1, 0, 0, 1),
                     (p(out), p(buf), 4, 0, too_big, None, 0, 1, 0, 0, 0), (p(out), p(buf), 4, 0, tau, None, 0, 1, 0, 4, 0)):
            assert tr(*args, C.byref(idx)) == zk.lib.ERR_BAD_ARGS, args
        for args in ((None, 4, 1, 1, 0, key, 0, 0, None, 0, p(s), p(sx)), (p(buf), 4, 1, 1, 0, None, 0, 0, None, 0, p(s), p(sx)),
                     (p(buf), 4, 1, 1, 0, key, 0, 0, None, 0, None, p(sx)), (p(buf), 1 << 31, 1, 1, 0, key, 0, 0, None, 0, p(s), p(sx)),
                     (p(buf), 4, 1, 1, 0, key, 0, 0, None, 1, p(s), p(sx))):
            assert pp(*args, C.byref(idx)) == zk.lib.ERR_BAD_ARGS, args
        assert tr(p(out), p(buf), 0, 0, tau, None, 0, 1, 0, 0, 0, C.byref(idx)) == 0 and idx.value == -1   # nothing to do


@pytest.mark.parametrize("group", [1, 2])
def test_transform_at_the_default_piece_size(zk, worker, group):
    """piece = 0 (2^18 points) and n = 2 * 2^18 + 5: three pieces, a ragged tail; against decode_points -> batch_exp over scalar_powers ->
    encode_points in memory, byte for byte"""
    import torch

    n, first = 2 * (1 << 18) + 5, 7
    tau, coeff = 0x123456789ABCDEF0123456789 % M.R_ORDER, 0xFEDCBA9876543210F % M.R_ORDER
    one = zk.keys.point_to_uncompressed(zk.ceremony.G1_ONE_RAW if group == 1 else zk.ceremony.G2_ONE_RAW)
    wire = np.tile(np.frombuffer(one, dtype=np.uint8), n)
    out = np.zeros(n * 32 * group, dtype=np.uint8)
    idx = C.c_longlong(0)
    lim = lambda v: (C.c_uint64 * 4)(*[(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)])  # noqa: E731
    rc = getattr(zk.lib.load(), f"mi355zk_bn254_g{group}_accumulator_transform")(
        out.ctypes.data_as(C.c_void_p), wire.ctypes.data_as(C.c_void_p), n, first, lim(tau), lim(coeff), 0, 1, 0, 0, 0, C.byref(idx))
    assert (rc, idx.value) == (0, -1)
    pts = zk.ceremony.decode_points(torch.from_numpy(wire).cuda().view(n, 64 * group), group, False, checked=False)
    exps = zk.ceremony.scalar_powers(tau, n, pts.device, coeff=coeff * pow(tau, first, M.R_ORDER) % M.R_ORDER)
    want = zk.ceremony.encode_points(zk.ceremony.batch_exp(pts, exps), True)
    assert np.array_equal(out, _np(want).reshape(-1))
