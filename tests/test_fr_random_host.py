"""The Fr scalar stream of csrc/chacha.hpp run on the host (mi355zk_selftest_fr_random; no device) against an independent pure-Python
ChaCha20 (tests/ceremony_model.py), and that model against the published keystream."""
import ctypes as C

import numpy as np
import pytest

import ceremony_model as CM

KEYS = ([0] * 8, [0x03020100, 0x07060504, 0x0B0A0908, 0x0F0E0D0C, 0x13121110, 0x17161514, 0x1B1A1918, 0xFFFFFFFF])
STREAMS = (0, 0x0123456789ABCDEF)
FIRSTS = (0, 1, (1 << 32) - 1, 1 << 32, (1 << 33) + 1)     # the counter's carry into word 13 ((2^33 + 1) >> 1 = 2^32), odd starts
COUNTS = (0, 1, 2, 3, 64, 65)


def _host(zk, n, key, stream_id, first):
    out = np.zeros((n, 4), np.uint64)
    rc = zk.lib.load().mi355zk_selftest_fr_random(out.ctypes.data_as(C.c_void_p), n, (C.c_uint32 * 8)(*key), stream_id, first)
    assert rc == 0
    return out


def test_the_model_reproduces_the_published_keystream(zk):
    """zero key, zero nonce, block 0: 76 b8 e0 ad a0 f1 3d 90 40 5d 6a e5 53 86 bd 28 ... (the first test vector of the ChaCha20 drafts)"""
    words = CM.chacha20_block([0] * 8, 0, 0)
    assert words[:4] == [0xADE0B876, 0x903DF1A0, 0xE56A5D40, 0x28BD8653]
    assert b"".join(w.to_bytes(4, "little") for w in words[:4]).hex() == "76b8e0ada0f13d90405d6ae55386bd28"
    got = _host(zk, 1, [0] * 8, 0, 0)[0]
    assert [int(v) for v in got[:2]] == [0x903DF1A0ADE0B876, 0x28BD8653E56A5D40]
    assert int(got[3]) == ((words[6] | words[7] << 32) & ((1 << 61) - 1))


@pytest.mark.parametrize("key", KEYS, ids=("zero_key", "key"))
@pytest.mark.parametrize("stream_id", STREAMS)
def test_host_stream_equals_the_model(zk, key, stream_id):
    for first in FIRSTS:
        for n in COUNTS:
            got = _host(zk, n, key, stream_id, first)
            want = np.array(CM.fr_random(key, stream_id, first, n), dtype=np.uint64).reshape(n, 4)
            assert got.tobytes() == want.tobytes(), (first, n)
            assert all(int(v) < (1 << 61) for v in got[:, 3])     # every value below 2^253


def test_keys_and_streams_differ(zk):
    base = _host(zk, 4, KEYS[1], 0, 0)
    assert not np.array_equal(base, _host(zk, 4, KEYS[0], 0, 0))
    assert not np.array_equal(base, _host(zk, 4, KEYS[1], 1, 0))
    assert not np.array_equal(base, _host(zk, 4, KEYS[1], 1 << 32, 0))     # the high word of the stream id is word 15


def test_a_range_is_the_concatenation_of_its_halves(zk):
    for first, n, cut in ((0, 65, 32), (1, 64, 33), ((1 << 32) - 1, 65, 1), (7, 10, 5)):
        whole = _host(zk, n, KEYS[1], 5, first)
        halves = np.concatenate([_host(zk, cut, KEYS[1], 5, first), _host(zk, n - cut, KEYS[1], 5, first + cut)])
        assert np.array_equal(whole, halves), (first, n, cut)


def test_bad_arguments(zk):
    lib = zk.lib.load()
    key = (C.c_uint32 * 8)()
    out = np.zeros((1, 4), np.uint64)
    assert lib.mi355zk_selftest_fr_random(None, 1, key, 0, 0) == zk.lib.ERR_BAD_ARGS
    assert lib.mi355zk_selftest_fr_random(out.ctypes.data_as(C.c_void_p), 1, None, 0, 0) == zk.lib.ERR_BAD_ARGS
    assert lib.mi355zk_selftest_fr_random(out.ctypes.data_as(C.c_void_p), 1 << 31, key, 0, 0) == zk.lib.ERR_BAD_ARGS
    assert lib.mi355zk_bn254_fr_random_dev(None, 1, key, 0, 0, None) == zk.lib.ERR_BAD_ARGS
    assert lib.mi355zk_bn254_fr_random_dev(out.ctypes.data_as(C.c_void_p), 1 << 31, key, 0, 0, None) == zk.lib.ERR_BAD_ARGS
    pt = np.zeros(12, np.uint64)
    assert lib.mi355zk_bn254_g1_merge_pairs_random_dev(None, None, 4, key, 0, None, pt.ctypes.data_as(C.c_void_p), pt.ctypes.data_as(C.c_void_p)) == zk.lib.ERR_BAD_ARGS
    assert lib.mi355zk_bn254_g1_merge_pairs_random(None, None, 4, key, 0, pt.ctypes.data_as(C.c_void_p), pt.ctypes.data_as(C.c_void_p)) == zk.lib.ERR_BAD_ARGS
    assert (1 << 253) < 21888242871839275222246405745257275088548364400416034343698204186575808495617 < (1 << 254)    # r >> 253 == 1: no rejection needed
