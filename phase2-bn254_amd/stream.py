"""Powers-of-tau files streamed through the device in bounded memory: the reference's `*_constrained` binaries, file to file.

  powersoftau/src/bin/new_constrained.rs               new_constrained(path, power, batch_size)
  powersoftau/src/bin/compute_constrained.rs           compute_constrained(challenge, response, power, batch_size, ...)
  powersoftau/src/bin/verify_transform_constrained.rs  verify_transform_constrained(challenge, response, new_challenge, power, batch_size, ...)

The reference's only accumulator is BatchedAccumulator over mmap'ed files (batched_accumulator.rs:394-531, 553-600, 1187-1290): a power-28
challenge is ~103 GB.  verify.contribute_response / read_response / next_challenge hold a whole file in HBM after several whole-file copies on
the host; the functions here map the files (numpy.memmap) and hand one chunk of one vector at a time -- a pointer into the mapping -- to
mi355zk_bn254_g{1,2}_accumulator_transform / _accumulator_power_pairs, which decode and encode the wire records on the device in pieces of
`piece` points.  Neither device nor host memory grows with the power: the device holds two pieces per call in flight, the host the pages of
the mappings the kernel keeps resident.  Results are those of the in-memory flows, byte for byte.

Chunks (`batches`) are the reference's: the index ranges 0 .. 2^p and 2^p .. 2^(p+1) - 1, each cut every batch_size elements.  Up to
_DEVICE_THREADS chunks are in flight at a time (one host thread each: one chunk's upload overlaps another's kernels and a third's download),
and one more thread hashes a file meanwhile (BLAKE2b releases the interpreter lock): four helper threads at most.

The random exponents of a verification are indexed GLOBALLY (scalar start + i of the vector's stream for the pair (v[start + i],
v[start + i + 1])), so the partial sums of the chunks add up to exactly the two points ceremony.power_pairs_random gives for the whole vector.
"""
from __future__ import annotations

import collections
import ctypes as C
import hashlib
import os
from concurrent.futures import ThreadPoolExecutor

import numpy as np

from . import ceremony, keys
from . import lib as _lib
from . import prover as _prover
from . import verify as _verify
from .bellman import DeviceError
from .ceremony import DeserializationError, GroupDecodingError
from .verify import VerificationError

_DEVICE_THREADS = 2
_HASH_SLICE = 1 << 30   # utils.rs:20-27 hashes the mapping in 1 GiB slices

# One chunk of one vector.  `count` elements from `start` are OWNED by the chunk (every index of every vector is owned exactly once: what a
# contribution transforms and a verification re-encodes); a verification reads `verify_count` records from `start`: one more than it owns
# unless it ends its range (batched_accumulator.rs:394-397, 465-475), so that consecutive chunks share a record and every pair of neighbours
# lies inside one chunk.  The pair across the two ranges of tau_g1 -- (2^p - 1, 2^p), which the reference checks from two saved elements
# (:456-458, 524-526, 533-540) -- is an entry of its own that owns nothing.  Offsets are the byte positions of element `start` in a
# compressed (response) and an uncompressed (challenge) file.
Batch = collections.namedtuple("Batch", "vector group start count verify_count compressed_offset uncompressed_offset")


def challenge_size(power: int) -> int:
    """bytes of a challenge: the uncompressed accumulator (parameters.rs:74-105 accumulator_size)"""
    return ceremony.accumulator_layout(power, False)[1]


def response_size(power: int) -> int:
    """bytes of a response: the compressed accumulator and the public key (contribution_size)"""
    return ceremony.accumulator_layout(power, True)[1] + keys.PUBLIC_KEY_SIZE


def batches(power: int, batch_size: int):
    """The reference's chunk plan as a list of Batch, in its order: the chunks of 0 .. 2^p (all five vectors), the junction pair of tau_g1,
    the chunks of 2^p .. 2^(p+1) - 1 (tau_g1 alone).  batch_size < 2 is refused: the reference panics on a one-element chunk."""
    if power < 0 or batch_size < 2:
        raise ValueError("batches: power >= 0 and batch_size >= 2")
    n = 1 << power
    lay_c = {name: (g, off) for name, g, _, off in ceremony.accumulator_layout(power, True)[0]}
    lay_u = {name: off for name, _, _, off in ceremony.accumulator_layout(power, False)[0]}
    out = []

    def entry(name, start, count, verify_count):
        g, off_c = lay_c[name]
        out.append(Batch(name, g, start, count, verify_count, off_c + start * ceremony._ENC_SIZE[(g, True)],
                         lay_u[name] + start * ceremony._ENC_SIZE[(g, False)]))

    for lo, hi, names in ((0, n, ("tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2")), (n, 2 * n - 1, ("tau_g1",))):
        for start in range(lo, hi, batch_size):
            end = min(start + batch_size, hi)
            for name in names:
                if name == "beta_g2":
                    if start == 0:
                        entry(name, 0, 1, 1)
                else:
                    entry(name, start, end - start, end - start + (0 if end == hi else 1))
        if lo == 0 and 2 * n - 1 > n:
            entry("tau_g1", n - 1, 0, 2)
    return out


def calculate_hash_file(path) -> bytes:
    """powersoftau/src/utils.rs:20-27: BLAKE2b-512 over the mapped file, 1 GiB at a time.  No copy of the file is made and hashlib releases
    the interpreter lock, so a helper thread can hash while the device works."""
    h = hashlib.blake2b(digest_size=64)
    if os.path.getsize(path):
        data = np.memmap(path, dtype=np.uint8, mode="r")
        for lo in range(0, data.shape[0], _HASH_SLICE):
            h.update(memoryview(data[lo:lo + _HASH_SLICE]))
        del data
    return h.digest()


def _check_size(path, want: int, what: str):
    have = os.path.getsize(path)
    if have != want:
        raise ValueError(f"{what} {path}: {have} bytes, a file of this power has {want}")


def new_constrained(path, power: int, batch_size: int) -> bytes:
    """new_constrained.rs:42-77: the initial challenge -- blank_hash(), then every element of every vector the group generator, uncompressed
    (BatchedAccumulator::generate_initial, batched_accumulator.rs:1295-1347) -- written chunk by chunk.  Byte-identical to
    ceremony.write_accumulator(ceremony.new_accumulator(power), compressed=False).  Returns the file's hash."""
    one = {1: np.frombuffer(keys.point_to_uncompressed(ceremony.G1_ONE_RAW), dtype=np.uint8),
           2: np.frombuffer(keys.point_to_uncompressed(ceremony.G2_ONE_RAW), dtype=np.uint8)}
    plan = batches(power, batch_size)
    out = np.memmap(path, dtype=np.uint8, mode="w+", shape=(challenge_size(power),))
    try:
        out[:ceremony.HASH_SIZE] = np.frombuffer(ceremony.blank_hash(), dtype=np.uint8)
        for b in plan:
            if b.count:
                out[b.uncompressed_offset:b.uncompressed_offset + b.count * one[b.group].size] = np.tile(one[b.group], b.count)
        out.flush()
    finally:
        del out
    return calculate_hash_file(path)


def _raise_for(rc: int, index: int, b: Batch, what: str):
    """the exception of the in-memory flow for a non-zero return of an accumulator entry point (indices are those of the whole vector)"""
    if rc == 5:
        raise VerificationError("g2 subgroup")
    if rc in GroupDecodingError.KINDS:
        raise GroupDecodingError(rc, b.start + index)
    if rc == _lib.ERR_POINT_AT_INFINITY:
        raise DeserializationError(f"PointAtInfinity in {b.vector}")
    if rc == _lib.ERR_BAD_ARGS:
        raise ValueError(f"{what}: bad arguments for {b.vector}[{b.start}:{b.start + max(b.count, b.verify_count)}]")
    raise DeviceError(f"{what} failed (rc={rc})")


def _limbs(v: int):
    return (C.c_uint64 * 4)(*[(v >> (64 * i)) & ((1 << 64) - 1) for i in range(4)])


def _run(jobs):
    """the chunks' device calls, at most _DEVICE_THREADS at a time on the caller's device; the results in plan order"""
    import torch

    dev = torch.cuda.current_device()
    with ThreadPoolExecutor(max_workers=_DEVICE_THREADS, initializer=torch.cuda.set_device, initargs=(dev,)) as pool:
        return list(pool.map(lambda job: job(), jobs))


def compute_constrained(challenge_path, response_path, power: int, batch_size: int, tau: int = None, alpha: int = None, beta: int = None,
                        piece: int = 0):
    """compute_constrained.rs: challenge file -> response file.  The challenge is read uncompressed and unchecked, the response written
    compressed (:14-16): its challenge's hash, tau_g1 / tau_g2 by tau^i, alpha_g1 / beta_g1 by alpha tau^i / beta tau^i, beta_g2 by beta
    (BatchedAccumulator::transform, batched_accumulator.rs:1187-1290), the public key.  One accumulator_transform call per chunk and vector,
    the challenge hashed meanwhile.  tau / alpha / beta: the private key, from the `secrets` module when None.  piece: points per device piece
    (0: the library's 2^18).  Returns (public key, the response's hash).  The response file is removed when the call fails."""
    L = _lib.load()
    _check_size(challenge_path, challenge_size(power), "challenge")
    plan = [b for b in batches(power, batch_size) if b.count]
    r = ceremony._R_ORDER
    priv = {"tau": tau, "alpha": alpha, "beta": beta}
    priv = {k: (v if v is not None else keys._random_scalar()) % r for k, v in priv.items()}
    coeff = {"tau_g1": None, "tau_g2": None, "alpha_g1": priv["alpha"], "beta_g1": priv["beta"], "beta_g2": priv["beta"]}
    tau_limbs = _limbs(priv["tau"])
    src = np.memmap(challenge_path, dtype=np.uint8, mode="r")
    dst = np.memmap(response_path, dtype=np.uint8, mode="w+", shape=(response_size(power),))
    ok = False
    try:
        src_at, dst_at = src.ctypes.data, dst.ctypes.data

        def job(b: Batch):
            def call():
                idx = C.c_longlong(-1)
                c = coeff[b.vector]
                rc = getattr(L, f"mi355zk_bn254_g{b.group}_accumulator_transform")(
                    C.c_void_p(dst_at + b.compressed_offset), C.c_void_p(src_at + b.uncompressed_offset), b.count, b.start, tau_limbs,
                    _limbs(c) if c is not None else None, 0, 1, 0, 0, piece, C.byref(idx))
                return rc, idx.value
            return call

        with ThreadPoolExecutor(max_workers=1) as hasher:
            digest_f = hasher.submit(calculate_hash_file, challenge_path)
            results = _run([job(b) for b in plan])
            digest = digest_f.result()
        for b, (rc, idx) in zip(plan, results):
            if rc:
                _raise_for(rc, idx, b, "compute_constrained")
        pub, _ = keys.keypair(digest, priv["tau"], priv["alpha"], priv["beta"])
        body = response_size(power) - keys.PUBLIC_KEY_SIZE
        dst[:ceremony.HASH_SIZE] = np.frombuffer(digest, dtype=np.uint8)
        dst[body:] = np.frombuffer(keys.write_public_key(pub), dtype=np.uint8)
        dst.flush()
        ok = True
    finally:
        del src, dst
        if not ok and os.path.exists(response_path):
            os.remove(response_path)
    return pub, calculate_hash_file(response_path)


def _record(data: np.ndarray, offset: int, group: int, index: int = 0):
    """one uncompressed record of a mapped file as a raw affine host record (checked; never the point at infinity)"""
    size = 64 * group
    return keys.point_from_uncompressed(bytes(data[offset:offset + size]), group, index)


def verify_transform_constrained(challenge_path, response_path, new_challenge_path, power: int, batch_size: int, key: bytes = None,
                                 check_g2_subgroup: bool = True, piece: int = 0):
    """verify_transform_constrained.rs: the response is the challenge transformed by the holder of the public key at its end; on success the
    next challenge -- the response's accumulator uncompressed, headed by the response's hash -- is written.  Returns (the response's hash,
    the new challenge's hash).

    Sizes, then the response's first 64 bytes against the challenge's hash (:113-138; VerificationError("challenge hash"), before any device
    work), the public key, the G2 points of the key and of the challenge's beta_g2 (check_g2_subgroup).  Then one accumulator_power_pairs
    call per chunk and vector over the compressed response (checked; tau_g2 / beta_g2 tested for membership), which also writes the chunk
    uncompressed into the new challenge; the chunks' sums are added on the host.  The eleven same_ratio checks are those of
    verify.verify_transform, decided in its one pairing launch and read in its order; failures raise what the in-memory flow raises
    (VerificationError(check), GroupDecodingError(kind, index in the vector), DeserializationError) and remove the new challenge.
    key: 32 bytes replacing os.urandom for the exponents (stream ids as in verify_transform: one per vector)."""
    import torch

    L = _lib.load()
    _check_size(challenge_path, challenge_size(power), "challenge")
    _check_size(response_path, response_size(power), "response")
    body = response_size(power) - keys.PUBLIC_KEY_SIZE
    resp = np.memmap(response_path, dtype=np.uint8, mode="r")
    chal = np.memmap(challenge_path, dtype=np.uint8, mode="r")
    new = None
    ok = False
    try:
        with ThreadPoolExecutor(max_workers=1) as hasher:
            digest = calculate_hash_file(challenge_path)
            if bytes(resp[:ceremony.HASH_SIZE]) != digest:
                raise VerificationError("challenge hash")
            response_hash_f = hasher.submit(calculate_hash_file, response_path)
            pk = keys.read_public_key(bytes(resp[body:]))
            lay_u = {name: off for name, _, _, off in ceremony.accumulator_layout(power, False)[0]}
            before = {"tau_g1": [_record(chal, lay_u["tau_g1"] + 64 * i, 1, i) for i in range(2)], "alpha_g1": [_record(chal, lay_u["alpha_g1"], 1)],
                      "beta_g1": [_record(chal, lay_u["beta_g1"], 1)], "beta_g2": [_record(chal, lay_u["beta_g2"], 2)]}
            device = torch.device("cuda", torch.cuda.current_device())
            if check_g2_subgroup:
                pts = np.stack([before["beta_g2"][0], pk["tau_g2"], pk["alpha_g2"], pk["beta_g2"]])
                with torch.cuda.device(device):
                    _verify._fail_unless(ceremony.g2_subgroup_check(torch.from_numpy(pts.view(np.int64)).to(device)) < 0, "g2 subgroup")
            ex = _verify._Exponents(key)
            streams = {name: ex.take() for name in ("tau_g1", "tau_g2", "alpha_g1", "beta_g1")}
            streams["beta_g2"] = (bytes(32), 0)   # (one element: no pair, no exponent is drawn)
            keys_c = {name: ceremony._chacha_key(k) for name, (k, _) in streams.items()}
            plan = batches(power, batch_size)
            new = np.memmap(new_challenge_path, dtype=np.uint8, mode="w+", shape=(challenge_size(power),))
            resp_at, new_at = resp.ctypes.data, new.ctypes.data

            def job(b: Batch):
                def call():
                    idx = C.c_longlong(-1)
                    s, sx = np.zeros(12 * b.group, dtype=np.uint64), np.zeros(12 * b.group, dtype=np.uint64)
                    rc = getattr(L, f"mi355zk_bn254_g{b.group}_accumulator_power_pairs")(
                        C.c_void_p(resp_at + b.compressed_offset), b.verify_count, 1, 1, 1 if check_g2_subgroup else 0, keys_c[b.vector],
                        streams[b.vector][1], b.start, C.c_void_p(new_at + b.uncompressed_offset) if b.count else None, piece,
                        s.ctypes.data_as(C.c_void_p), sx.ctypes.data_as(C.c_void_p), C.byref(idx))
                    return rc, idx.value, s, sx
                return call

            results = _run([job(b) for b in plan])
            sums = {}
            for b, (rc, idx, s, sx) in zip(plan, results):
                if rc:
                    _raise_for(rc, idx, b, "verify_transform_constrained")
                sums[b.vector] = (s, sx) if b.vector not in sums else (_prover._add(sums[b.vector][0], s), _prover._add(sums[b.vector][1], sx))
            powers = {name: (_prover._to_affine(sums[name][0]), _prover._to_affine(sums[name][1])) for name in ("tau_g1", "tau_g2", "alpha_g1", "beta_g1")}
            # the response's first records, from the uncompressed copy the device has just written
            after = {name: [_record(new, lay_u[name] + 64 * g * i, g, i) for i in range(2 if name in ("tau_g1", "tau_g2") else 1)]
                     for name, g in (("tau_g1", 1), ("tau_g2", 2), ("alpha_g1", 1), ("beta_g1", 1), ("beta_g2", 2))}
            _verify._decide_transform(device, pk, digest, before, after, powers)
            response_hash = response_hash_f.result()
        new[:ceremony.HASH_SIZE] = np.frombuffer(response_hash, dtype=np.uint8)
        new.flush()
        ok = True
    finally:
        del resp, chal, new
        if not ok and os.path.exists(new_challenge_path):
            os.remove(new_challenge_path)
    return response_hash, calculate_hash_file(new_challenge_path)
