"""mi355zk_bn254_g{1,2}_points_load / _points_store (csrc/accumulator_stream.hip): wire records in host memory <-> one device vector, in
pieces.  The compressed tau_g1 (31 records) and tau_g2 (16) of a power-4 response against ceremony.decode_points / encode_points, with
pieces of 3 records (ragged last piece, both buffer sets reused) and the library's 2^18; a refused record, an infinity and a G2 record
outside the subgroup in the SECOND piece give their code and their index within the call."""
import ctypes as C

import numpy as np
import pytest

import bn254_model as M
import ceremony_model as CM

pytestmark = pytest.mark.gpu

POWER = 4
SECRETS = (0xABCDEF123456789, 0x1111222233334444, 0x9999AAAABBBB)
VECTORS = {"tau_g1": (1, 31), "tau_g2": (2, 16)}


def _np(t) -> np.ndarray:
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def wire(zk, worker):
    """{vector: the compressed records of a power-4 response as a host uint8 array}"""
    import torch

    challenge = _np(zk.ceremony.write_accumulator(zk.ceremony.new_accumulator(POWER, torch.device("cuda", 0)), compressed=False)).tobytes()
    response = _np(zk.contribute_response(challenge, POWER, *SECRETS)[0])
    layout = {name: (g, cnt, off) for name, g, cnt, off in zk.ceremony.accumulator_layout(POWER, True)[0]}
    return {name: response[layout[name][2]:layout[name][2] + cnt * 32 * g].copy() for name, (g, cnt) in VECTORS.items()}


@pytest.mark.parametrize("piece", [3, 0])
@pytest.mark.parametrize("vector", list(VECTORS))
def test_load_then_store_is_decode_then_encode(zk, worker, wire, vector, piece):
    import torch

    g, n = VECTORS[vector]
    data = wire[vector]
    want = zk.ceremony.decode_points(torch.from_numpy(data).cuda().view(n, 32 * g), g, True)
    got = zk.points_load(data, g, n, True, True, g == 2, piece, vector)
    assert got.shape == (n, 8 * g) and torch.equal(got, want)
    for compressed in (True, False):
        size = (32 if compressed else 64) * g
        out = np.full(n * size + 8, 0xEE, dtype=np.uint8)
        zk.points_store(out[:n * size], got, compressed, piece)
        assert np.array_equal(out[:n * size], _np(zk.ceremony.encode_points(want, compressed)).reshape(-1))
        assert (out[n * size:] == 0xEE).all()
        back = zk.points_load(out[:n * size], g, n, compressed, False, False, piece)
        assert torch.equal(back, want)


def test_infinity_is_stored_as_the_codec_writes_it(zk, worker):
    import torch

    for g in (1, 2):
        pts = torch.zeros((5, 8 * g), dtype=torch.int64, device="cuda")
        for compressed in (True, False):
            out = np.zeros(5 * (32 if compressed else 64) * g, dtype=np.uint8)
            zk.points_store(out, pts, compressed, 2)
            assert np.array_equal(out, _np(zk.ceremony.encode_points(pts, compressed)).reshape(-1))
            assert out[0] == 0x40
            with pytest.raises(zk.ceremony.DeserializationError):
                zk.points_load(out, g, 5, compressed, True, False, 2, "v")


def _off_subgroup_g2() -> np.ndarray:
    """a point of the twist outside the order-r subgroup, as tests/test_gpu_stream.py makes one"""
    for c in range(1, 50):
        x = (c, 0)
        y = CM.f2_sqrt(M.f2_add(M.f2_mul(M.f2_mul(x, x), x), M.B_G2))
        if y is not None and M.ec_mul(M.FQ2_OPS, (x, y), M.R_ORDER) is not None:
            return np.array(M.g2_affine_to_raw((x, y)), dtype=np.uint64)
    raise AssertionError("no point found")


def _load(zk, group, data, n, piece, check_subgroup=0):
    import torch

    out = torch.zeros((n, 8 * group), dtype=torch.int64, device="cuda")
    torch.cuda.synchronize()
    idx = C.c_longlong(-7)
    rc = getattr(zk.lib.load(), f"mi355zk_bn254_g{group}_points_load")(C.c_void_p(out.data_ptr()), data.ctypes.data_as(C.c_void_p), n, 1, 1, check_subgroup,
                                                                     piece, C.byref(idx))
    return rc, idx.value


def test_bad_records_in_the_second_piece_give_their_code_and_index(zk, worker, wire):
    import torch

    for vector, (g, n) in VECTORS.items():
        size = 32 * g
        assert _load(zk, g, wire[vector], n, 3, 1) == (0, -1)
        for record, code, exc in ((M.Q.to_bytes(32, "big") + bytes(size - 32), 6, zk.ceremony.GroupDecodingError),
                                  (bytes([0x40]) + bytes(size - 1), zk.lib.ERR_POINT_AT_INFINITY, zk.ceremony.DeserializationError)):
            bad = wire[vector].copy()
            bad[4 * size:5 * size] = np.frombuffer(record, dtype=np.uint8)   # pieces of 3: record 4 is the second record of the second piece
            bad[9 * size:10 * size] = np.frombuffer(record, dtype=np.uint8)  # a later piece is never looked at
            assert _load(zk, g, bad, n, 3) == (code, 4)
            assert _load(zk, g, bad, n, 0) == (code, 4)
            with pytest.raises(exc) as e:
                zk.points_load(bad, g, n, True, True, False, 3, vector)
            if exc is zk.ceremony.GroupDecodingError:
                assert (e.value.kind, e.value.index) == ("CoordinateDecodingError", 4)
            else:
                assert vector in str(e.value)
    g, n = VECTORS["tau_g2"]
    bad = wire["tau_g2"].copy()
    off = _np(zk.ceremony.encode_points(torch.from_numpy(_off_subgroup_g2().view(np.int64).reshape(1, 16)).cuda(), True)).reshape(-1)
    bad[5 * 64:6 * 64] = off
    assert _load(zk, g, bad, n, 3, check_subgroup=1) == (5, 5)
    assert _load(zk, g, bad, n, 3, check_subgroup=0) == (0, -1)       # on the twist: the decoder admits it, as the reference's does
    with pytest.raises(zk.VerificationError) as e:
        zk.points_load(bad, g, n, True, True, True, 3, "tau_g2")
    assert e.value.check == "g2 subgroup"


def test_argument_checks(zk, worker):
    import torch

    L = zk.lib.load()
    bad = zk.lib.ERR_BAD_ARGS
    host = np.zeros(4 * 128, dtype=np.uint8)
    dev = torch.zeros((5, 16), dtype=torch.int64, device="cuda")
    idx = C.c_longlong(0)
    p = host.ctypes.data_as(C.c_void_p)
    for g in (1, 2):
        load, store = getattr(L, f"mi355zk_bn254_g{g}_points_load"), getattr(L, f"mi355zk_bn254_g{g}_points_store")
        assert load(None, p, 4, 0, 0, 0, 0, C.byref(idx)) == bad
        assert load(C.c_void_p(dev.data_ptr()), None, 4, 0, 0, 0, 0, C.byref(idx)) == bad
        assert load(C.c_void_p(dev.data_ptr() + 8), p, 4, 0, 0, 0, 0, C.byref(idx)) == bad
        assert load(C.c_void_p(dev.data_ptr()), p, 4, 0, 0, 0, 1 << 31, C.byref(idx)) == bad
        assert load(None, None, 0, 0, 0, 0, 0, C.byref(idx)) == 0 and idx.value == -1
        assert load(None, None, 0, 0, 0, 0, 0, None) == 0
        assert store(None, C.c_void_p(dev.data_ptr()), 4, 0, 0) == bad
        assert store(p, None, 4, 0, 0) == bad
        assert store(p, C.c_void_p(dev.data_ptr() + 8), 4, 0, 0) == bad
        assert store(p, C.c_void_p(dev.data_ptr()), 4, 0, 1 << 31) == bad
        assert store(None, None, 0, 0, 0) == 0
    with pytest.raises(ValueError):
        zk.points_load(host[:100], 1, 4, True)                        # too few bytes
    with pytest.raises(ValueError):
        zk.points_store(host[:100], dev[:, :8].contiguous(), False)
