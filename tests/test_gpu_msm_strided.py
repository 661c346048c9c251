"""Strided affine records on the GPU (include/mi355zk.h: mi355zk_bn254_g{1,2}_msm_strided, mi355zk_bases_cache_pin_strided,
mi355zk_bn254_g{1,2}_records_pack_dev): base vectors in the caller's layout -- pairing's `G1Affine { x, y, infinity: bool }` (72 B) /
G2Affine (136 B) and other layouts of the same fields -- give exactly the result, return code and error index of the packed host
entry on the same points, and the CPU oracle's.  Padding bytes are garbage (0xA5); flagged records hold the reference's identity
encoding x = 0, y = R (ec.rs:163-169), which only the flag byte marks as infinity."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import golden_util as GU
import inputs
import oracle_lib as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Q = 21888242871839275222246405745257275088696311157297823662689037894645226208583
R_MONT = [((1 << 256) % Q >> (64 * i)) & ((1 << 64) - 1) for i in range(4)]   # Fq::one() in Montgomery form


def _G(group):
    return O.G1 if group == 1 else O.G2


def encode(zk, packed, group, stride, x_off, y_off, inf_off=None, flags=None, pad=0xA5):
    """numpy: packed (n, 8 / 16) u64 records -> a StridedBases of the given layout; flagged records get x = 0, y = R."""
    n, csz = packed.shape[0], 32 * group
    raw = packed.view(np.uint8).reshape(n, 2 * csz).copy()
    if flags is not None and flags.any():
        one = np.zeros(csz, np.uint8)
        one[:32] = np.array(R_MONT, dtype=np.uint64).view(np.uint8)
        raw[flags, :csz] = 0
        raw[flags, csz:] = one
    data = np.full((n, stride), pad, dtype=np.uint8)
    data[:, x_off:x_off + csz] = raw[:, :csz]
    data[:, y_off:y_off + csz] = raw[:, csz:]
    if inf_off is not None:
        data[:, inf_off] = 0 if flags is None else flags.astype(np.uint8)
    return zk.StridedBases(data, group, x_off, y_off, inf_off)


def zeroed(packed, flags):
    out = packed.copy()
    out[flags] = 0
    return out


def layouts(group):
    """(stride, x_off, y_off, inf_off): the Rust layout, flag byte first, y before x, a wider record without a flag, the packed one"""
    c = 32 * group
    return [(2 * c + 8, 0, c, 2 * c), (2 * c + 8, 8, 8 + c, 0), (2 * c + 8, c, 0, 2 * c), (2 * c + 16, 8, 12 + c, None), (2 * c, 0, c, None)]


def _aff(group, fut):
    return _G(group).to_affine(fut.wait())


@pytest.mark.parametrize("group", [1, 2])
@pytest.mark.parametrize("n", [1, 100, 4096])
def test_rust_layout_matches_packed_and_oracle(zk, worker, group, n):
    rng = np.random.default_rng(7000 + n + group)
    packed = inputs.bases_progression_cpu(group, n, seed=7001 + group)
    flags = rng.random(n) < 0.1
    if n == 1:
        flags[:] = False
    scalars = inputs.random_scalars(n, seed=7002 + n)
    scalars[flags] = 0
    sb = zk.StridedBases.g1_affine_rust if group == 1 else zk.StridedBases.g2_affine_rust
    limbs = 4 * group
    x, y = packed[:, :limbs].copy(), packed[:, limbs:].copy()
    x[flags], y[flags] = 0, 0
    y[flags, 0:4] = R_MONT
    bases = sb(x, y, flags, pad=0xA5)
    assert bases.data.shape == (n, 72 if group == 1 else 136)
    want_packed = _aff(group, zk.multiexp(worker, (zeroed(packed, flags), 0), zk.FullDensity(), scalars))
    got = _aff(group, zk.multiexp(worker, (bases, 0), zk.FullDensity(), scalars))
    assert np.array_equal(got, want_packed)
    rc, want = _G(group).multiexp(zeroed(packed, flags), scalars, threads=4)
    assert rc == 0 and np.array_equal(got, _G(group).to_affine(want))
    if flags.any():  # a flagged base under a non-zero exponent: UnexpectedIdentity at the packed call's index
        i = int(np.nonzero(flags)[0][-1])
        scalars[i] = np.array([3, 0, 0, 0], dtype=np.uint64)
        errs = []
        for b in (zeroed(packed, flags), bases):
            with pytest.raises(zk.SynthesisError) as e:
                zk.multiexp(worker, (b, 0), zk.FullDensity(), scalars).wait()
            errs.append((e.value.kind, e.value.index))
        assert errs[0] == errs[1] == (zk.SynthesisError.UNEXPECTED_IDENTITY, i)


@pytest.mark.parametrize("group", [1, 2])
def test_other_layouts_give_the_packed_result(zk, worker, group):
    n = 700
    rng = np.random.default_rng(7100 + group)
    packed = inputs.bases_progression_cpu(group, n, seed=7101 + group)
    scalars = inputs.random_scalars(n, seed=7102)
    flags = rng.random(n) < 0.2
    scalars[flags] = 0
    want = _aff(group, zk.multiexp(worker, (zeroed(packed, flags), 0), zk.FullDensity(), scalars))
    for stride, xo, yo, io in layouts(group):
        f = flags if io is not None else None
        b = encode(zk, zeroed(packed, flags) if io is None else packed, group, stride, xo, yo, io, f)
        assert np.array_equal(_aff(group, zk.multiexp(worker, (b, 0), zk.FullDensity(), scalars)), want), (stride, xo, yo, io)


@pytest.mark.parametrize("group", [1, 2])
def test_density_offset_and_eof(zk, worker, group):
    n, off = 1500, 5
    rng = np.random.default_rng(7200 + group)
    bits = rng.random(n) < 0.5
    used = int(bits.sum())
    packed = inputs.bases_progression_cpu(group, used + off, seed=7201)
    scalars = inputs.random_scalars(n, seed=7202)
    scalars[::17] = 0
    b = encode(zk, packed, group, *layouts(group)[0], flags=np.zeros(used + off, bool))
    rc, want = _G(group).multiexp(packed, scalars, density=GU.density_words(bits), density_bits=n, base_offset=off, threads=4)
    assert rc == 0
    got = _aff(group, zk.multiexp(worker, (b, off), zk.DensityTracker.from_bools(bits), scalars))
    assert np.array_equal(got, _G(group).to_affine(want))
    # one base short: UnexpectedEof at the packed call's index
    short_p, short_s = packed[:used + off - 1], zk.StridedBases(b.data[:used + off - 1], group, b.x_off, b.y_off, b.inf_off)
    errs = []
    for bb in (short_p, short_s):
        with pytest.raises(zk.SynthesisError) as e:
            zk.multiexp(worker, (bb, off), zk.DensityTracker.from_bools(bits), scalars).wait()
        errs.append((e.value.kind, e.value.index))
    assert errs[0] == errs[1] and errs[0][0] == zk.SynthesisError.IO_UNEXPECTED_EOF


@pytest.mark.parametrize("group", [1, 2])
def test_streamed_upload_matches_the_oracle(zk, worker, group, monkeypatch):
    monkeypatch.setenv("MI355ZK_HOST_CHUNK_TEST", "512")
    n, off = 3000, 7
    rng = np.random.default_rng(7300 + group)
    packed = inputs.bases_progression_cpu(group, n + off, seed=7301)
    flags = rng.random(n + off) < 0.05
    scalars = inputs.random_scalars(n, seed=7302)
    scalars[flags[off:]] = 0
    rc, want = _G(group).multiexp(zeroed(packed, flags), scalars, base_offset=off, threads=4)
    assert rc == 0
    want = _G(group).to_affine(want)
    b = encode(zk, packed, group, *layouts(group)[0], flags=flags)
    assert np.array_equal(_aff(group, zk.multiexp(worker, (b, off), zk.FullDensity(), scalars)), want)
    zk.pin_bases(b)   # the first pinned call uploads chunk by chunk and then completes the entry around the consumed range
    try:
        for _ in range(2):
            assert np.array_equal(_aff(group, zk.multiexp(worker, (b, off), zk.FullDensity(), scalars)), want)
        d, t = C.c_size_t(), C.c_size_t()
        assert zk.lib.load().mi355zk_bases_cache_info(b.ptr(), C.byref(d), C.byref(t)) == 1 and d.value == (n + off) * 64 * group
    finally:
        zk.unpin_bases(b)


def test_natural_2e23_call_matches_packed(zk, worker):
    """2^23 exponents: the natural chunking of an uploading call (bases travel), raw pieces repacked as they arrive"""
    from test_gpu_msm import _dev_inputs

    bases, scalars, _ = _dev_inputs(zk, 23, seed=7401)
    hb, hs = bases.cpu().numpy().view(np.uint64), scalars.cpu().numpy().view(np.uint64)
    del bases, scalars
    want = _aff(1, zk.multiexp(worker, (hb, 0), zk.FullDensity(), hs))
    b = zk.StridedBases.g1_affine_rust(hb[:, :4], hb[:, 4:], None, pad=0xA5)
    del hb
    assert np.array_equal(_aff(1, zk.multiexp(worker, (b, 0), zk.FullDensity(), hs)), want)


@pytest.mark.parametrize("group", [1, 2])
def test_pinning(zk, worker, group):
    n = 4000
    rng = np.random.default_rng(7500 + group)
    packed = inputs.bases_progression_cpu(group, n, seed=7501)
    flags = rng.random(n) < 0.1
    scalars = inputs.random_scalars(n, seed=7502)
    scalars[flags] = 0
    lib = zk.lib.load()
    want = _aff(group, zk.multiexp(worker, (zeroed(packed, flags), 0), zk.FullDensity(), scalars))
    b = encode(zk, packed, group, *layouts(group)[0], flags=flags)
    d, t = C.c_size_t(), C.c_size_t()
    zk.pin_bases(b)
    try:
        for _ in range(2):
            assert np.array_equal(_aff(group, zk.multiexp(worker, (b, 0), zk.FullDensity(), scalars)), want)
        assert lib.mi355zk_bases_cache_info(b.ptr(), C.byref(d), C.byref(t)) == 1
        assert d.value == n * 64 * group and t.value == 0
        # a second layout at the same pointer (the flag ignored: stride 72 / 136, x 0, y 32 / 64, no flag) is its own entry
        other = zk.StridedBases(b.data, group, 0, 32 * group, None)
        zk.pin_bases(other)
        sc2 = scalars.copy()
        sc2[flags] = 0
        assert np.array_equal(_aff(group, zk.multiexp(worker, (other, 0), zk.FullDensity(), sc2)), want)  # the flagged records, x = 0 y = R, are skipped (exponent 0)
        assert lib.mi355zk_bases_cache_info(b.ptr(), C.byref(d), C.byref(t)) == 1 and d.value == 2 * n * 64 * group
        assert np.array_equal(_aff(group, zk.multiexp(worker, (b, 0), zk.FullDensity(), scalars)), want)
    finally:
        zk.unpin_bases(b)
    assert lib.mi355zk_bases_cache_info(b.ptr(), C.byref(d), C.byref(t)) == 0
    # after unpin, a flag byte rewritten in place is seen
    i = int(np.nonzero(~flags)[0][3])
    b.data[i, b.inf_off] = 1
    with pytest.raises(zk.SynthesisError) as e:
        zk.multiexp(worker, (b, 0), zk.FullDensity(), scalars).wait()
    assert e.value.kind == zk.SynthesisError.UNEXPECTED_IDENTITY and e.value.index == i
    b.data[i, b.inf_off] = 0
    # PIN_TABLES: the second call runs in table mode from the packed entry, same result
    zk.pin_bases(b, tables=True)
    try:
        for _ in range(3):
            assert np.array_equal(_aff(group, zk.multiexp(worker, (b, 0), zk.FullDensity(), scalars)), want)
        assert lib.mi355zk_bases_cache_info(b.ptr(), C.byref(d), C.byref(t)) == 1 and d.value == n * 64 * group and t.value > 0
    finally:
        zk.unpin_bases(b)


@pytest.mark.parametrize("group", [1, 2])
def test_logical_devices_slices_of_a_pinned_strided_vector(zk, worker, group, monkeypatch):
    n, off = 3000, 3
    rng = np.random.default_rng(7600 + group)
    bits = rng.random(n) < 0.7
    used = int(bits.sum())
    packed = inputs.bases_progression_cpu(group, used + off, seed=7601)
    flags = rng.random(used + off) < 0.05
    scalars = inputs.random_scalars(n, seed=7602)
    scalars[:] = 0
    scalars[bits] = inputs.random_scalars(used, seed=7603)
    scalars[np.nonzero(bits)[0][flags[off:]]] = 0     # exponents of flagged bases
    b = encode(zk, packed, group, *layouts(group)[0], flags=flags)
    dm = zk.DensityTracker.from_bools(bits)
    want = _aff(group, zk.multiexp(worker, (b, off), dm, scalars))
    assert np.array_equal(want, _aff(group, zk.multiexp(worker, (zeroed(packed, flags), off), dm, scalars)))
    monkeypatch.setenv("MI355ZK_MULTI_MIN_LOG", "6")
    try:
        w = zk.Worker(devices=[0] * 4)
        assert zk.lib.load().mi355zk_device_count() == 4
        zk.pin_bases(b)
        for _ in range(2):
            assert np.array_equal(_aff(group, zk.multiexp(w, (b, off), dm, scalars)), want)
        d, t = C.c_size_t(), C.c_size_t()
        assert zk.lib.load().mi355zk_bases_cache_info(b.ptr(), C.byref(d), C.byref(t)) == 1 and 0 < d.value <= (used + off) * 64 * group
    finally:
        zk.unpin_bases(None)
        zk.Worker(0)
    assert zk.lib.load().mi355zk_device_count() == 1


@pytest.mark.parametrize("group", [1, 2])
def test_records_pack_dev_is_byte_exact(zk, worker, group):
    import torch

    n = 100_000
    c = 32 * group
    lib = zk.lib.load()
    fn = lib.mi355zk_bn254_g1_records_pack_dev if group == 1 else lib.mi355zk_bn254_g2_records_pack_dev
    rng = np.random.default_rng(7700 + group)
    dev = torch.device("cuda", 0)
    out = torch.empty((n, 2 * c), dtype=torch.uint8, device=dev)
    for stride, xo, yo, io in layouts(group):
        raw = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
        if io is not None:
            raw[:, io] = np.where(rng.random(n) < 0.3, rng.integers(1, 256, size=n), 0)
        want = np.concatenate([raw[:, xo:xo + c], raw[:, yo:yo + c]], axis=1)
        if io is not None:
            want[raw[:, io] != 0] = 0
        d_raw = torch.from_numpy(raw).to(dev)
        out.fill_(0x5A)
        rc = fn(C.c_void_p(d_raw.data_ptr()), n, stride, xo, yo, zk.lib.NO_FLAG if io is None else io, C.c_void_p(out.data_ptr()),
                C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want), (stride, xo, yo, io)
    # aliasing input and output is refused
    assert fn(C.c_void_p(out.data_ptr()), 16, 2 * c + 8, 0, c, 2 * c, C.c_void_p(out.data_ptr()), None) == 3


def test_cpp_program_pins_shared_records(zk, worker):
    from test_msm_strided_host import build_cpp

    exe = build_cpp()
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stdout + out.stderr
    for name in ("strided_g1_rust_layout", "strided_g2_rust_layout", "strided_pinned_shared_ptr", "strided_identity_error"):
        assert "ok " + name in out.stdout, out.stdout
