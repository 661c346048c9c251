"""stream.prepare_phase2_files: a power-4 response (or challenge) file -> every phase1radix2m{k}, against the in-memory flow
ceremony.prepare_phase2 (the sparse-product H bases: the independent path) and against the closed forms from the secrets through the CPU
oracle's scalar multiplication.  Secrets that drive the H bases through the doubling and the infinity branch, the degree filter, the
failures (which leave no file) and the way back through read_phase1radix2m_file into circom.mpc_parameters_new."""
import os

import numpy as np
import pytest

import bn254_model as M
import ceremony_model as CM
import inputs
import oracle_lib as O
import prepare_phase2_cases as P

pytestmark = pytest.mark.gpu

POWER = 4
SECRETS1 = (0xABCDEF123456789, 0x1111222233334444, 0x9999AAAABBBB)     # as tests/test_gpu_stream.py
ROOT16 = pow(M.FR_ROOT_OF_UNITY, 1 << (M.FR_S - 4), M.R_ORDER)        # a primitive 16th root of unity in Fr
SECRETS_ROOT = (ROOT16, 0x89ABCDEF01, 0x55AA55AA55)


def _np(t) -> np.ndarray:
    return t.cpu().numpy()


def _dev(a):
    import torch

    a = np.array(a)
    return torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a).cuda()


def _limbs(v):
    return np.array(M.to_limbs(v % M.R_ORDER), dtype=np.uint64)


@pytest.fixture(scope="module")
def files(zk, worker, tmp_path_factory):
    """the fresh challenge (tau = alpha = beta = 1) and two responses to it, as bytes and as files"""
    import torch

    d = tmp_path_factory.mktemp("prepare")
    out = {"dir": d}
    out["challenge0"] = _np(zk.ceremony.write_accumulator(zk.ceremony.new_accumulator(POWER, torch.device("cuda", 0)), compressed=False)).tobytes()
    out["response1"] = _np(zk.contribute_response(out["challenge0"], POWER, *SECRETS1)[0]).tobytes()
    out["response_root"] = _np(zk.contribute_response(out["challenge0"], POWER, *SECRETS_ROOT)[0]).tobytes()
    for name in ("challenge0", "response1", "response_root"):
        (d / name).write_bytes(out[name])
    return out


def _in_memory(zk, data: bytes, compressed: bool, k: int) -> bytes:
    acc = zk.ceremony.read_accumulator(_dev(np.frombuffer(data, dtype=np.uint8)), POWER, compressed)
    return _np(zk.ceremony.write_phase1radix2m(zk.ceremony.prepare_phase2(acc, 1 << k))).tobytes()


def _closed_form(zk, secrets, k: int) -> bytes:
    """the file of degree 2^k from the secrets: every record is its scalar times the generator (the oracle's scalar multiplication and codec)"""
    scalars = P.radix_scalars(*secrets, 1 << k)
    out = b""
    for name, g, _ in zk.ceremony._RADIX_FIELDS:
        if not scalars[name]:
            continue
        G, gen = (O.G1, inputs.G1_GEN_RAW) if g == 1 else (O.G2, inputs.G2_GEN_RAW)
        pts = G.mul_many_affine(gen, np.stack([_limbs(s) for s in scalars[name]]))
        out += O.encode_points(g, pts, False).tobytes()
    return out


@pytest.fixture(scope="module")
def full_run(zk, worker, files):
    """every degree of response 1 at the library's piece size: {k: bytes}"""
    d = files["dir"] / "full"
    paths = zk.prepare_phase2_files(files["dir"] / "response1", d, POWER)
    assert sorted(paths) == list(range(POWER + 1)) and sorted(os.listdir(d)) == sorted(f"phase1radix2m{k}" for k in range(POWER + 1))
    return {k: open(p, "rb").read() for k, p in paths.items()}


def test_generic_secrets_give_the_in_memory_files_and_the_closed_form(zk, worker, files, full_run, tmp_path):
    want = {k: _in_memory(zk, files["response1"], True, k) for k in range(POWER + 1)}
    for k in range(POWER + 1):
        assert len(full_run[k]) == 256 + 320 * (1 << k) + 64 * ((1 << k) - 1)
        assert full_run[k] == want[k], k
    paths = zk.prepare_phase2_files(files["dir"] / "response1", tmp_path, POWER, piece=3)     # ragged pieces, both buffer sets reused
    for k in range(POWER + 1):
        assert str(paths[k]) == str(tmp_path / f"phase1radix2m{k}")
        assert open(paths[k], "rb").read() == want[k], k
    assert full_run[3] == _closed_form(zk, SECRETS1, 3)


def test_a_root_of_unity_tau_takes_the_doubling_and_the_infinity_branches(zk, worker, files, tmp_path):
    """tau^8 = -1: tau_g1[i + 8] = -tau_g1[i], every H base of degree 8 is a doubling; tau^16 = 1: every H base of degree 16 is infinity and
    L_j(tau) = [j == 1], so the Lagrange vectors of degree 16 are infinity but for one record.  The closed form decides."""
    assert pow(ROOT16, 8, M.R_ORDER) == M.R_ORDER - 1 and pow(ROOT16, 16, M.R_ORDER) == 1
    assert P.lagrange_at(ROOT16, 16) == [0, 1] + [0] * 14
    paths = zk.prepare_phase2_files(files["dir"] / "response_root", tmp_path, POWER, degrees=[3, 4], piece=5)
    assert sorted(paths) == [3, 4]
    for k in (3, 4):
        got = open(paths[k], "rb").read()
        assert got == _closed_form(zk, SECRETS_ROOT, k), k
    h16 = got[-15 * 64:]
    assert h16 == (bytes([0x40]) + bytes(63)) * 15                    # infinity as the codec writes it


def test_the_fresh_challenge_is_read_uncompressed(zk, worker, files, tmp_path):
    """tau = 1: every H base is infinity (equal operands) and only L_0 is non-zero"""
    paths = zk.prepare_phase2_files(files["dir"] / "challenge0", tmp_path, POWER, compressed=False, checked=False, piece=4)
    for k in range(POWER + 1):
        assert open(paths[k], "rb").read() == _closed_form(zk, (1, 1, 1), k), k


def test_the_degree_filter_writes_that_file_only(zk, worker, files, full_run, tmp_path):
    paths = zk.prepare_phase2_files(files["dir"] / "response1", tmp_path / "sub", POWER, degrees=[2, 2])
    assert list(paths) == [2] and os.listdir(tmp_path / "sub") == ["phase1radix2m2"]
    assert open(paths[2], "rb").read() == full_run[2]
    # without the membership test at load the G2 transforms run untrusted: the same bytes
    paths = zk.prepare_phase2_files(files["dir"] / "response1", tmp_path / "plain", POWER, degrees=[2], check_g2_subgroup=False)
    assert open(paths[2], "rb").read() == full_run[2]
    with pytest.raises(ValueError):
        zk.prepare_phase2_files(files["dir"] / "response1", tmp_path / "none", POWER, degrees=[5])
    assert not (tmp_path / "none").exists()


def _with_record(data: bytes, offset: int, record: bytes) -> bytes:
    return data[:offset] + record + data[offset + len(record):]


def _off_subgroup_g2() -> np.ndarray:
    """a point of the twist outside the order-r subgroup, as tests/test_gpu_stream.py makes one"""
    for c in range(1, 50):
        x = (c, 0)
        y = CM.f2_sqrt(M.f2_add(M.f2_mul(M.f2_mul(x, x), x), M.B_G2))
        if y is not None and M.ec_mul(M.FQ2_OPS, (x, y), M.R_ORDER) is not None:
            return np.array(M.g2_affine_to_raw((x, y)), dtype=np.uint64)
    raise AssertionError("no point found")


def test_failures_raise_and_leave_no_file(zk, worker, files, tmp_path):
    layout = {name: off for name, _, _, off in zk.ceremony.accumulator_layout(POWER, True)[0]}
    out = tmp_path / "out"
    out.mkdir()
    # a truncated input
    (tmp_path / "short").write_bytes(files["response1"][:-1])
    with pytest.raises(ValueError):
        zk.prepare_phase2_files(tmp_path / "short", out, POWER)
    with pytest.raises(ValueError):
        zk.prepare_phase2_files(files["dir"] / "response1", out, POWER, compressed=False)    # a response is no challenge
    assert os.listdir(out) == []
    # an existing output path: refused before any work, and the file is left as it was
    (out / "phase1radix2m3").write_bytes(b"mine")
    with pytest.raises(FileExistsError):
        zk.prepare_phase2_files(files["dir"] / "response1", out, POWER)
    assert os.listdir(out) == ["phase1radix2m3"] and (out / "phase1radix2m3").read_bytes() == b"mine"
    os.remove(out / "phase1radix2m3")
    # a corrupted record in alpha_g1, in the third piece
    (tmp_path / "bad").write_bytes(_with_record(files["response1"], layout["alpha_g1"] + 32 * 7, M.Q.to_bytes(32, "big")))
    with pytest.raises(zk.ceremony.GroupDecodingError) as e:
        zk.prepare_phase2_files(tmp_path / "bad", out, POWER, piece=3)
    assert (e.value.kind, e.value.index) == ("CoordinateDecodingError", 7)
    assert os.listdir(out) == []
    # the point at infinity in beta_g1
    (tmp_path / "inf").write_bytes(_with_record(files["response1"], layout["beta_g1"] + 32 * 2, bytes([0x40]) + bytes(31)))
    with pytest.raises(zk.ceremony.DeserializationError) as e:
        zk.prepare_phase2_files(tmp_path / "inf", out, POWER)
    assert "beta_g1" in str(e.value) and os.listdir(out) == []
    # a G2 record outside the subgroup
    import torch

    off = _np(zk.ceremony.encode_points(torch.from_numpy(_off_subgroup_g2().view(np.int64).reshape(1, 16)).cuda(), True)).tobytes()
    (tmp_path / "g2").write_bytes(_with_record(files["response1"], layout["tau_g2"] + 64 * 11, off))
    with pytest.raises(zk.VerificationError) as e:
        zk.prepare_phase2_files(tmp_path / "g2", out, POWER, piece=3)
    assert e.value.check == "g2 subgroup" and os.listdir(out) == []


def test_a_written_file_reads_back_into_phase2(zk, worker, files, full_run, tmp_path):
    import torch

    m = 8
    path = tmp_path / "phase1radix2m3"
    path.write_bytes(full_run[3])
    got = zk.read_phase1radix2m_file(path, m)
    want = zk.ceremony.read_phase1radix2m(_dev(np.frombuffer(full_run[3], dtype=np.uint8)), m)
    assert list(got) == list(want)
    for name in want:
        assert torch.equal(got[name], want[name]), name
    r = M.R_ORDER
    circuit_json = {   # x1 * x2 = x3;  (x3 + 5) * 1 = out: the circuit of tests/test_gpu_verify.py
        "constraints": [[{"2": "1"}, {"3": "1"}, {"4": "1"}], [{"4": "1", "0": "5"}, {"0": "1"}, {"1": str(r - 1), "0": "0"}]],
        "nPubInputs": 1, "nOutputs": 1, "nVars": 5}
    circuit = zk.circom.circuit_from_json(circuit_json)
    assert 1 << zk.circom.domain_exponent(zk.circom.assemble(circuit).num_constraints) == m
    from_file = zk.circom.mpc_parameters_new(circuit, False, got)
    in_memory = zk.circom.mpc_parameters_new(circuit, False, zk.ceremony.prepare_phase2(
        zk.ceremony.read_accumulator(_dev(np.frombuffer(files["response1"], dtype=np.uint8)), POWER, True), m))
    assert _np(zk.ceremony.write_mpc_parameters(from_file)).tobytes() == _np(zk.ceremony.write_mpc_parameters(in_memory)).tobytes()
    # sizes are checked against the plan's
    with pytest.raises(ValueError):
        zk.read_phase1radix2m_file(path, 16)
    with pytest.raises(ValueError):
        zk.read_phase1radix2m_file(path, 6)
    # a file with an infinity record is refused, as parameters.rs:164 does
    (tmp_path / "inf").write_bytes(_with_record(full_run[3], 256 + 64 * 2, bytes([0x40]) + bytes(63)))
    with pytest.raises(zk.ceremony.DeserializationError) as e:
        zk.read_phase1radix2m_file(tmp_path / "inf", m)
    assert "coeffs_g1" in str(e.value)
