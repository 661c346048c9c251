"""Powers-of-tau files streamed through the device in bounded memory: the reference's `*_constrained` binaries, file to file.

  powersoftau/src/bin/new_constrained.rs               new_constrained(path, power, batch_size)
  powersoftau/src/bin/compute_constrained.rs           compute_constrained(challenge, response, power, batch_size, ...)
  powersoftau/src/bin/verify_transform_constrained.rs  verify_transform_constrained(challenge, response, new_challenge, power, batch_size, ...)
  powersoftau/src/bin/prepare_phase2.rs                prepare_phase2_files(response, out_dir, power, degrees, ...) over prepare_phase2_plan;
                                                       read_phase1radix2m_file reads a result back (the second half of this module)

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


# ---------------------------------------------------------------------------------------------------------------
# prepare_phase2, file to files (powersoftau/src/bin/prepare_phase2.rs): a response (or challenge) -> phase1radix2m{k} for every degree.
# Whole VECTORS cross the link here, not chunks: a point ifft needs its 2^k inputs together.  mi355zk_bn254_g{1,2}_points_load decodes a
# vector's prefix from the mapping into one device tensor, in pieces; points_store encodes a device tensor into a mapping.

PlanLoad = collections.namedtuple("PlanLoad", "vector group count offset")       # `count` records from byte `offset` of the input file
PlanSection = collections.namedtuple("PlanSection", "name group count offset")   # a section of an output file
PlanFile = collections.namedtuple("PlanFile", "size sections")                   # sections: {name: PlanSection}, in _RADIX_FIELDS' order
# the Lagrange sections each source vector feeds
_RADIX_SOURCES = (("tau_g1", "coeffs_g1"), ("tau_g2", "coeffs_g2"), ("alpha_g1", "alpha_coeffs_g1"), ("beta_g1", "beta_coeffs_g1"))
# bytes per point of a point transform's scratch (working point, Z coordinate, window-table entry) and its lanes per launch, G1 / G2
_PFFT_SCRATCH = {1: (112, 32, 192, 1 << 20), 2: (224, 64, 368, 1 << 19)}


def _al256(x: int) -> int:
    return (x + 255) & ~255


def radix_file_layout(m: int) -> PlanFile:
    """phase1radix2m{log2 m}: the sections of ceremony._RADIX_FIELDS, uncompressed, back to back: 256 + 320 m + 64 (m - 1) bytes"""
    off, sections = 0, collections.OrderedDict()
    for name, g, cnt in ceremony._RADIX_FIELDS:
        sections[name] = PlanSection(name, g, cnt(m), off)
        off += cnt(m) * ceremony._ENC_SIZE[(g, False)]
    return PlanFile(off, sections)


class Phase2Plan:
    """What prepare_phase2_files does, as host arithmetic (prepare_phase2_plan builds it):

      power, compressed, degrees (sorted, distinct), kmax, input_size
      loads   {vector: PlanLoad} in the order the vectors are loaded: the prefix every degree needs, loaded ONCE
      files   {k: PlanFile}
      order   the steps, in order: ("load", vector), ("head", section), ("ifft", vector, k, section), ("h", k), ("free", vector)
    """

    def __init__(self, power, compressed, degrees, input_size, loads, files, order):
        self.power, self.compressed, self.degrees, self.kmax, self.input_size = power, compressed, degrees, degrees[-1], input_size
        self.loads, self.files, self.order = loads, files, order

    def device_bytes(self, piece: int = 0) -> int:
        """The peak device memory of the flow beyond what the process held before, for pieces of `piece` records (0: lib.POINTS_PIECE).
        One source vector is resident at a time, with n = 2^kmax and R = 64 / 128 B the raw record of its group:

          the vector          count * R        (count = 2 n - 1 for tau_g1, n otherwise)
          the work buffer     n * R            (every degree's copy, and then its H bases, are views of this one buffer)
          point_ifft at n     n * W + (n / 2 + 1) * 32 + n * Z + 8 * min(n, LANES) * T, each term rounded up to 256 B: working points,
                              twiddles, Z coordinates and the window table (W, Z, T = 112, 32, 192 B and LANES = 2^20 for G1; 224, 64, 368 B
                              and 2^19 for G2) -- allocated and freed by every transform, largest at kmax
                              + n B for a G2 transform's membership flags (counted always: check_g2_subgroup=False runs the test per call)

        and the maximum over the vectors is taken (G2 at equal n: 256 n against G1's 192 n - 64).  Next to it the ONE pooled buffer of
        points_load / points_store, which is leased by one call at a time and grows to the largest request: with P = min(piece, count)

          load    2 * (P * in_record + P [G2] + 256)        store   2 * P * R

        (include/mi355zk.h), the maximum over all calls.  The shifted difference allocates nothing.  torch's allocator is asked to return
        its cached blocks after every vector, so what one vector held is not still held under the next.  On top of the resident sum goes
        1 / 32 of it for what the allocators and the runtime add (rounding of every allocation, page tables): an allowance, not a
        derivation -- the low-water mark of free device memory lay 1.7 % above the sum at 2^20 and 0.6 % at 2^18 (profiles/prepare_phase2.md).
        One-time costs of the process (code objects, streams) are not counted."""
        piece = piece or _lib.POINTS_PIECE
        n = 1 << self.kmax
        peak = lease = 0
        for ld in self.loads.values():
            rec = 64 * ld.group
            in_rec = ceremony._ENC_SIZE[(ld.group, self.compressed)]
            p = min(piece, ld.count)
            lease = max(lease, 2 * (_al256(p * in_rec) + (_al256(p) if ld.group == 2 else 0) + 256))
            held = ld.count * rec
            if ld.vector != "beta_g2":
                w, z, t, lanes = _PFFT_SCRATCH[ld.group]
                held += n * rec + _al256(n * w) + _al256((n // 2 + 1) * 32) + _al256(n * z) + 8 * min(n, lanes) * t + (n if ld.group == 2 else 0)
                lease = max(lease, 2 * _al256(min(piece, n) * rec))
            peak = max(peak, held)
        return peak + peak // 32 + lease


def prepare_phase2_plan(power: int, degrees=None, compressed: bool = True) -> Phase2Plan:
    """The plan of prepare_phase2_files for an accumulator file of `power`.  degrees: the exponents k of the files phase1radix2m{k} to
    write; None: every k in 0 .. power, the reference's loop (prepare_phase2.rs:60).  0 <= k <= power, duplicates collapse; anything else
    raises ValueError.  Every source vector is loaded once, as the prefix the LARGEST degree needs -- 2^kmax records, 2^(kmax + 1) - 1 of
    tau_g1 (the H bases reach m - 1 places past m) -- and every smaller degree works on a prefix of that."""
    if isinstance(power, bool) or not isinstance(power, int) or not 0 <= power <= 28:
        raise ValueError("prepare_phase2_plan: 0 <= power <= 28")
    if degrees is None:
        degrees = range(power + 1)
    degrees = list(degrees)
    if not degrees or any(isinstance(k, bool) or not isinstance(k, (int, np.integer)) or not 0 <= k <= power for k in degrees):
        raise ValueError(f"prepare_phase2_plan: degrees are exponents k with 0 <= k <= {power}, at least one")
    degrees = tuple(sorted({int(k) for k in degrees}))
    kmax = degrees[-1]
    layout, body = ceremony.accumulator_layout(power, compressed)
    lay = {name: (g, cnt, off) for name, g, cnt, off in layout}
    want = {"tau_g1": (2 << kmax) - 1, "tau_g2": 1 << kmax, "alpha_g1": 1 << kmax, "beta_g1": 1 << kmax, "beta_g2": 1}
    loads = collections.OrderedDict((name, PlanLoad(name, lay[name][0], min(want[name], lay[name][1]), lay[name][2])) for name, _, _ in ceremony._ACC_FIELDS)
    files = collections.OrderedDict((k, radix_file_layout(1 << k)) for k in degrees)
    order = []
    for vector, section in _RADIX_SOURCES:
        order.append(("load", vector))
        if vector in ("alpha_g1", "beta_g1"):
            order.append(("head", vector))
        order += [("ifft", vector, k, section) for k in degrees]
        if vector == "tau_g1":
            order += [("h", k) for k in degrees if k > 0]
        order.append(("free", vector))
    order += [("load", "beta_g2"), ("head", "beta_g2"), ("free", "beta_g2")]
    return Phase2Plan(power, bool(compressed), degrees, body + (keys.PUBLIC_KEY_SIZE if compressed else 0), loads, files, order)


def _raise_points(rc: int, index: int, vector: str, what: str):
    """the stream module's exception for a non-zero return of points_load / points_store"""
    _raise_for(rc, index, Batch(vector, 0, 0, 0, 0, 0, 0), what)


def points_load(data: np.ndarray, group: int, count: int, compressed: bool, checked: bool = True, check_subgroup: bool = False, piece: int = 0,
                vector: str = "points"):
    """`count` wire records at the start of `data` (a contiguous uint8 host array, typically a slice of a mapping) -> a (count, 8 * group)
    int64 tensor of raw affine records on the current device: mi355zk_bn254_g{1,2}_points_load.  The current stream is synchronised first;
    the call returns when the tensor is complete.  Raises GroupDecodingError(kind, index), DeserializationError("PointAtInfinity in
    <vector>") or VerificationError("g2 subgroup") for the first piece that fails."""
    import torch

    size = ceremony._ENC_SIZE[(group, bool(compressed))]
    if data.dtype != np.uint8 or not data.flags["C_CONTIGUOUS"] or data.size < count * size:
        raise ValueError(f"points_load: {vector} needs {count * size} contiguous bytes")
    out = torch.empty((count, 8 * group), dtype=torch.int64, device=torch.device("cuda", torch.cuda.current_device()))
    torch.cuda.current_stream().synchronize()
    idx = C.c_longlong(-1)
    rc = getattr(_lib.load(), f"mi355zk_bn254_g{group}_points_load")(
        C.c_void_p(out.data_ptr()), C.c_void_p(data.ctypes.data), count, 1 if compressed else 0, 1 if checked else 0, 1 if check_subgroup else 0,
        piece, C.byref(idx))
    if rc:
        _raise_points(rc, idx.value, vector, "points_load")
    return out


def points_store(data: np.ndarray, points, compressed: bool, piece: int = 0):
    """The inverse: the (n, 8) / (n, 16) device records `points` encoded into the start of `data` (a writable contiguous uint8 host array):
    mi355zk_bn254_g{1,2}_points_store.  The current stream is synchronised first; the call returns when the bytes are in `data`."""
    import torch

    group = ceremony._group(points)
    n = points.shape[0]
    size = ceremony._ENC_SIZE[(group, bool(compressed))]
    if data.dtype != np.uint8 or not data.flags["C_CONTIGUOUS"] or not data.flags["WRITEABLE"] or data.size < n * size or not points.is_contiguous():
        raise ValueError(f"points_store: {n * size} writable contiguous bytes and contiguous records")
    torch.cuda.current_stream().synchronize()
    rc = getattr(_lib.load(), f"mi355zk_bn254_g{group}_points_store")(C.c_void_p(data.ctypes.data), C.c_void_p(points.data_ptr()), n,
                                                                    1 if compressed else 0, piece)
    if rc:
        _raise_points(rc, -1, "points", "points_store")


def prepare_phase2_files(path, out_dir, power: int, degrees=None, compressed: bool = True, checked: bool = True, check_g2_subgroup: bool = True,
                         piece: int = 0):
    """prepare_phase2.rs, file to files: the accumulator in `path` -> out_dir/phase1radix2m{k} for every k of `degrees` (None: 0 .. power, the
    reference's loop); returns {k: path}.  Each file is byte for byte ceremony.write_phase1radix2m(ceremony.prepare_phase2(acc, 2^k)).

    compressed=True: `path` is a response (compressed body + public key, response_size(power) bytes -- what the reference reads, with
    CheckForCorrectness::Yes = `checked`); False: a challenge (challenge_size(power)).  Another size raises ValueError.  The input is mapped,
    never read whole; the outputs are created at their final size (an existing one raises FileExistsError before any work: the reference's
    create_new) and mapped; every file this call created is removed when it fails.

    The work is vector-major (prepare_phase2_plan(...).order): each of tau_g1, tau_g2, alpha_g1, beta_g1 is uploaded and decoded ONCE, as the
    prefix the largest degree needs; then for every k its first 2^k records are copied, transformed (ceremony.point_ifft) and stored into
    that file's section -- for tau_g1 also the H bases tau_g1[i + 2^k] - tau_g1[i] (ceremony.shifted_difference) -- and the vector is
    freed.  alpha_g1[0], beta_g1[0] and beta_g2 head every file.  One vector is on the device at a time: Phase2Plan.device_bytes(piece).
    check_g2_subgroup: tau_g2 and beta_g2 are tested for membership at load (VerificationError("g2 subgroup")) and the G2 transforms run as
    trusted; False: no test at load, and point_ifft runs its own per call.  Only the prefixes that are loaded are decoded and checked: with
    degrees below `power` the rest of the file is not looked at.
    Raises GroupDecodingError(kind, index in the vector), DeserializationError("PointAtInfinity in <vector>"), VerificationError."""
    import torch

    plan = prepare_phase2_plan(power, degrees, compressed)
    _check_size(path, plan.input_size, "response" if compressed else "challenge")
    os.makedirs(out_dir, exist_ok=True)
    paths = collections.OrderedDict((k, os.path.join(out_dir, f"phase1radix2m{k}")) for k in plan.degrees)
    for p in paths.values():
        if os.path.lexists(p):
            raise FileExistsError(p)
    src = np.memmap(path, dtype=np.uint8, mode="r")
    outs, created = {}, []
    ok = False
    try:
        for k, p in paths.items():
            with open(p, "xb") as f:
                f.truncate(plan.files[k].size)
            created.append(p)
            outs[k] = np.memmap(p, dtype=np.uint8, mode="r+")

        def section(k, name):
            s = plan.files[k].sections[name]
            return outs[k][s.offset:s.offset + s.count * ceremony._ENC_SIZE[(s.group, False)]]

        vec = work = copy = None
        for step in plan.order:
            if step[0] == "load":
                ld = plan.loads[step[1]]
                in_size = ceremony._ENC_SIZE[(ld.group, plan.compressed)]
                vec = points_load(src[ld.offset:ld.offset + ld.count * in_size], ld.group, ld.count, plan.compressed, checked,
                                  check_g2_subgroup and ld.group == 2, piece, ld.vector)
                if ld.vector != "beta_g2":
                    work = torch.empty((1 << plan.kmax, 8 * ld.group), dtype=torch.int64, device=vec.device)
            elif step[0] == "head":
                for k in plan.degrees:
                    points_store(section(k, step[1]), vec[:1], False, piece)
            elif step[0] == "ifft":
                _, _, k, name = step
                copy = work[:1 << k]
                copy.copy_(vec[:1 << k])
                ceremony.point_ifft(copy, trusted_subgroup=bool(check_g2_subgroup))
                points_store(section(k, name), copy, False, piece)
            elif step[0] == "h":
                m = 1 << step[1]
                points_store(section(step[1], "h"), ceremony.shifted_difference(vec, m, m - 1, out=work), False, piece)
            else:   # "free" (the views too: one of them would keep the work buffer alive under the next vector)
                vec = work = copy = None
                torch.cuda.empty_cache()
        for o in outs.values():
            o.flush()
        ok = True
    finally:
        del src
        outs.clear()
        if not ok:
            for p in created:
                if os.path.exists(p):
                    os.remove(p)
    return dict(paths)


def read_phase1radix2m_file(path, m: int):
    """A phase1radix2m{log2 m} file -> the dict of raw affine device records ceremony.read_phase1radix2m gives for its bytes
    (phase2/src/parameters.rs:147-217: into_affine_unchecked, the point at infinity refused -> DeserializationError), loaded section by
    section from the mapping with points_load: no whole-file tensor, so circom.mpc_parameters_new can start from a file of any degree.
    ValueError when m is no power of two or the file's size is not that of degree m."""
    if isinstance(m, bool) or not isinstance(m, (int, np.integer)) or m < 1 or m & (m - 1):
        raise ValueError("read_phase1radix2m_file: m must be a power of two")
    lay = radix_file_layout(int(m))
    _check_size(path, lay.size, "phase1radix2m")
    src = np.memmap(path, dtype=np.uint8, mode="r")
    try:
        return {s.name: points_load(src[s.offset:s.offset + s.count * ceremony._ENC_SIZE[(s.group, False)]], s.group, s.count, False, False, False,
                                    0, s.name) for s in lay.sections.values()}
    finally:
        del src
