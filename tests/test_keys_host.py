"""phase2-bn254_amd/keys.py on the host (no device): hash_to_g2 against the big-int model's stored results, the two properties the
reference tests (powersoftau/src/utils.rs:53-74), membership of the result, the public-key records."""
import ctypes as C
import hashlib
import json
import os

import numpy as np
import pytest

import bn254_model as M
import ceremony_model as CM

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "hash_to_g2.json")))["cases"]


def _in_subgroup(zk, rec) -> bool:
    rec = np.ascontiguousarray(rec, dtype=np.uint64)
    return zk.lib.load().mi355zk_selftest_g2_in_subgroup(rec.ctypes.data_as(C.c_void_p)) == 1


@pytest.mark.parametrize("case", GOLDEN, ids=[c["digest"][:8] for c in GOLDEN])
def test_hash_to_g2_equals_the_model(zk, case):
    got = zk.keys.hash_to_g2(bytes.fromhex(case["digest"]))
    assert ["%016x" % int(v) for v in got] == case["g2"]
    p = M.g2_affine_from_raw(got)
    assert p is not None and M.on_curve_g2(p)          # non-zero, on the twist
    assert _in_subgroup(zk, got)
    assert M.ec_mul(M.FQ2_OPS, p, M.R_ORDER) is None   # the same statement by the model: r P = 0


def test_the_stored_results_are_the_models(zk):
    case = GOLDEN[0]
    assert M.g2_affine_to_raw(CM.hash_to_g2(bytes.fromhex(case["digest"]))) == [int(w, 16) for w in case["g2"]]


def test_hash_to_g2_reads_exactly_32_bytes(zk):
    """utils.rs:53-74: a 33rd byte is ignored, the 32nd is not"""
    d = bytes(range(1, 33))
    base = zk.keys.hash_to_g2(d)
    assert np.array_equal(zk.keys.hash_to_g2(d + bytes([33])), zk.keys.hash_to_g2(d + bytes([34])))
    assert np.array_equal(zk.keys.hash_to_g2(d + bytes([33])), base)
    assert not np.array_equal(zk.keys.hash_to_g2(d[:31] + bytes([33])), base)
    with pytest.raises(ValueError):
        zk.keys.hash_to_g2(d[:31])


def test_chacha_rng_is_the_keystream_word_by_word(zk):
    rng = zk.keys.ChaChaRng([0] * 8)
    first = [rng.next_u32() for _ in range(20)]
    assert first[:4] == [0xADE0B876, 0x903DF1A0, 0xE56A5D40, 0x28BD8653]
    assert first == CM.chacha20_block([0] * 8, 0)[:16] + CM.chacha20_block([0] * 8, 1)[:4]
    rng = zk.keys.ChaChaRng([0] * 8)
    assert rng.next_u64() == (0xADE0B876 << 32) | 0x903DF1A0      # the high word first


def test_compute_g2_s_is_the_hash_of_the_personalised_transcript(zk):
    digest = hashlib.blake2b(b"challenge", digest_size=64).digest()
    g1_s = np.array(M.g1_affine_to_raw(M.ec_mul(M.FQ_OPS, M.G1_GEN, 5)), dtype=np.uint64)
    g1_s_x = np.array(M.g1_affine_to_raw(M.ec_mul(M.FQ_OPS, M.G1_GEN, 35)), dtype=np.uint64)
    enc = lambda p: b"".join(v.to_bytes(32, "big") for v in p)  # noqa: E731
    for personalization in (0, 1, 2):
        h = hashlib.blake2b(bytes([personalization]) + digest + enc(M.ec_mul(M.FQ_OPS, M.G1_GEN, 5)) + enc(M.ec_mul(M.FQ_OPS, M.G1_GEN, 35)),
                            digest_size=64).digest()
        want = M.g2_affine_to_raw(CM.hash_to_g2(h))
        assert [int(v) for v in zk.keys.compute_g2_s(digest, g1_s, g1_s_x, personalization)] == want


def test_public_key_records_round_trip(zk):
    digest = hashlib.blake2b(b"", digest_size=64).digest()
    tau, alpha, beta = 0x1234567, 0x89ABCDEF01, 0x55AA55AA55
    pub, priv = zk.keys.keypair(digest, tau, alpha, beta)
    assert priv == {"tau": tau, "alpha": alpha, "beta": beta}
    blob = zk.keys.write_public_key(pub)
    assert len(blob) == zk.keys.PUBLIC_KEY_SIZE == 6 * 64 + 3 * 128
    back = zk.keys.read_public_key(blob)
    assert sorted(back) == sorted(pub) and all(np.array_equal(back[k], pub[k]) for k in pub)
    assert zk.keys.write_public_key(back) == blob
    # the proof of knowledge in the exponent: g1_s_x = x g1_s, and g2_s_x = x compute_g2_s(...)
    for name, x, pers in (("tau", tau, 0), ("alpha", alpha, 1), ("beta", beta, 2)):
        s, sx = M.g1_affine_from_raw(pub[f"{name}_g1_s"]), M.g1_affine_from_raw(pub[f"{name}_g1_s_{name}"])
        assert M.on_curve_g1(s) and M.ec_mul(M.FQ_OPS, s, x) == sx
        g2_s = M.g2_affine_from_raw(zk.keys.compute_g2_s(digest, pub[f"{name}_g1_s"], pub[f"{name}_g1_s_{name}"], pers))
        assert M.ec_mul(M.FQ2_OPS, g2_s, x) == M.g2_affine_from_raw(pub[f"{name}_g2"])
        assert _in_subgroup(zk, pub[f"{name}_g2"])
    # keys.rs: two key pairs for one digest differ (g1_s is drawn afresh)
    other, _ = zk.keys.keypair(digest, tau, alpha, beta)
    assert not np.array_equal(other["tau_g1_s"], pub["tau_g1_s"])


def test_public_key_reader_rejects_what_the_reference_rejects(zk):
    digest = bytes(64)
    pub, _ = zk.keys.keypair(digest, 3, 5, 7)
    blob = bytearray(zk.keys.write_public_key(pub))
    for off, size in ((0, 64), (64 * 5, 64), (384, 128), (384 + 256, 128)):
        bad = bytearray(blob)
        bad[off:off + size] = bytes(size)                       # an all-zero record: (0, 0) is not on the curve
        with pytest.raises(zk.ceremony.GroupDecodingError) as e:
            zk.keys.read_public_key(bytes(bad))
        assert e.value.kind == "NotOnCurve"
        bad[off] = 0x40                                          # the encoding of the point at infinity
        with pytest.raises(zk.ceremony.DeserializationError):
            zk.keys.read_public_key(bytes(bad))
    bad = bytearray(blob)
    bad[0] |= 0x80
    with pytest.raises(zk.ceremony.GroupDecodingError) as e:
        zk.keys.read_public_key(bytes(bad))
    assert e.value.kind == "UnexpectedCompressionMode"
    bad = bytearray(blob)
    bad[64:96] = (M.Q).to_bytes(32, "big")
    with pytest.raises(zk.ceremony.GroupDecodingError) as e:
        zk.keys.read_public_key(bytes(bad))
    assert e.value.kind == "CoordinateDecodingError" and e.value.index == 1
    with pytest.raises(ValueError):
        zk.keys.read_public_key(bytes(blob[:-1]))


def test_mpc_public_key_hash_is_blake2b_of_the_record(zk):
    pk = {"delta_after": np.array(M.g1_affine_to_raw(M.ec_mul(M.FQ_OPS, M.G1_GEN, 2)), dtype=np.uint64),
          "s": np.array(M.g1_affine_to_raw(M.ec_mul(M.FQ_OPS, M.G1_GEN, 3)), dtype=np.uint64),
          "s_delta": np.array(M.g1_affine_to_raw(M.ec_mul(M.FQ_OPS, M.G1_GEN, 6)), dtype=np.uint64),
          "r_delta": np.array(M.g2_affine_to_raw(M.ec_mul(M.FQ2_OPS, M.G2_GEN, 2)), dtype=np.uint64), "transcript": bytes(range(64))}
    enc1 = lambda p: b"".join(v.to_bytes(32, "big") for v in p)  # noqa: E731
    q = M.ec_mul(M.FQ2_OPS, M.G2_GEN, 2)
    want = (enc1(M.ec_mul(M.FQ_OPS, M.G1_GEN, 2)) + enc1(M.ec_mul(M.FQ_OPS, M.G1_GEN, 3)) + enc1(M.ec_mul(M.FQ_OPS, M.G1_GEN, 6))
            + b"".join(v.to_bytes(32, "big") for v in (q[0][1], q[0][0], q[1][1], q[1][0])) + bytes(range(64)))
    assert zk.keys.mpc_public_key_bytes(pk) == want
    assert zk.keys.mpc_public_key_hash(pk) == hashlib.blake2b(want, digest_size=64).digest()
