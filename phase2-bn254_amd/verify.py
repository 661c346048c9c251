"""The ceremony steps and their verification, assembled from the device pieces: what `phase2-bn254` exists for.

Mirrored interfaces (same names, argument meaning and order of the checks):
  phase2/src/parameters.rs:414-522              MPCParameters::contribute     -> contribute_mpc_parameters(mpc, delta)
  phase2/src/parameters.rs:726-854              verify_contribution(before, after)
  phase2/src/parameters.rs:529-659              MPCParameters::verify         -> verify_mpc_parameters(mpc, circuit, filter, radix)
  powersoftau/src/bin/compute_constrained.rs    challenge -> response          -> contribute_response(challenge_bytes, power)
  powersoftau/src/batched_accumulator.rs:182-272  verify_transform(before, after, key, digest)
  powersoftau/src/bin/verify_transform_constrained.rs  response -> new challenge  -> next_challenge(response_bytes, power)

ONE PAIRING LAUNCH PER VERIFICATION.  The reference runs its same_ratio checks one after the other and returns at the first that fails.  A
pairing launch costs the same latency for one pair as for a few thousand, so every same_ratio of a verification is collected into ONE
pairing.same_ratio_batch call -- 5 for verify_contribution, 2 k + 3 for verify_mpc_parameters over k contributions, 11 for
verify_transform -- and the verdicts are then read in the reference's order: the check reported is the one the reference would have
stopped at.  Lengths and byte equalities that the reference tests before its first pairing are tested before the launch, and fail before it.

RANDOM EXPONENTS.  Every merge_pairs / power_pairs takes its exponents from the device generator (ceremony.merge_pairs_random): a fresh
32-byte key from os.urandom per vector, a distinct stream_id per vector.  `key=` (32 bytes) replaces os.urandom for reproducible runs.

G2 MEMBERSHIP.  The device pairing is specified for G2 points of the order-r subgroup; the reference's decoders only test the curve
equation.  By default every G2 point that came from a file (r_delta, delta_g2, tau_g2, beta_g2, the key's G2 points) goes through
ceremony.g2_subgroup_check first and the verification fails with "g2 subgroup" if one is outside.  check_g2_subgroup=False skips the test
(the reference's behaviour): the verdict for a point outside the subgroup is then unspecified, nothing faults.

Failures raise VerificationError(check), `check` naming the failed test.
"""
from __future__ import annotations

import hashlib
import os

import numpy as np

from . import ceremony, circom, keys, pairing
from . import prover as _prover


class VerificationError(Exception):
    """A verification failed; .check names the reference's test that would have returned Err / false."""

    def __init__(self, check: str):
        super().__init__(f"verification failed: {check}")
        self.check = check


def _fail_unless(ok, check: str):
    if not ok:
        raise VerificationError(check)


def _bytes(x) -> bytes:
    return bytes(x.cpu().numpy()) if hasattr(x, "cpu") else bytes(x)


def _same(a, b) -> bool:
    """equality of two device vectors (lengths included), compared where they are"""
    import torch

    return a.shape == b.shape and torch.equal(a, b)


class _Exponents:
    """the key and stream id of each successive merge_pairs of one verification"""

    def __init__(self, key):
        if key is not None and len(bytes(key)) != 32:
            raise ValueError("key: 32 bytes")
        self.key, self.next_id = (bytes(key) if key is not None else None), 0

    def take(self):
        sid, self.next_id = self.next_id, self.next_id + 1
        return (self.key if self.key is not None else os.urandom(32)), sid


def _merged(v1, v2, ex: _Exponents):
    """merge_pairs as a pair of affine host records"""
    s, sx = ceremony.merge_pairs_random(v1.contiguous(), v2.contiguous(), *ex.take())
    return _prover._to_affine(s), _prover._to_affine(sx)


def _powers(v, ex: _Exponents):
    v = v.contiguous()
    s, sx = ceremony.power_pairs_random(v, *ex.take())
    return _prover._to_affine(s), _prover._to_affine(sx)


class _Ratios:
    """the same_ratio checks of one verification, in the reference's order, and the one launch that decides them"""

    def __init__(self, device):
        self.device, self.names, self.rows = device, [], []

    def add(self, check: str, g1_pair, g2_pair):
        """same_ratio(g1_pair, g2_pair) with the G1 pair first, as utils.rs:151-159 takes them when G1 = G1Affine"""
        self.names.append(check)
        self.rows.append((keys._host(g1_pair[0], 8), keys._host(g1_pair[1], 8), keys._host(g2_pair[0], 16), keys._host(g2_pair[1], 16)))

    def add_g2_first(self, check: str, g2_pair, g1_pair):
        """same_ratio(g2_pair, g1_pair) -- power_pairs over a G2 vector (batched_accumulator.rs:252-256): e(g1.1, g2.0) == e(g1.0, g2.1),
        the same statement with the roles exchanged"""
        self.add(check, g1_pair, g2_pair)

    def run(self) -> dict:
        """{check: verdict} from ONE pairing launch"""
        import torch

        cols = [np.stack([r[k] for r in self.rows]) for k in range(4)]
        dev = [torch.from_numpy(c.view(np.int64)).to(self.device) for c in cols]
        with torch.cuda.device(self.device):
            ok = pairing.same_ratio_batch(*dev)
        return dict(zip(self.names, (bool(v) for v in ok)))


def _subgroup(points, enabled: bool):
    """every G2 record of `points` (device tensors or host records) lies in the order-r subgroup, or VerificationError("g2 subgroup")"""
    import torch

    if not enabled:
        return
    dev = next(p.device for p in points if hasattr(p, "device") and getattr(p, "is_cuda", False))
    parts = [p.reshape(-1, 16) if getattr(p, "is_cuda", False) else torch.from_numpy(keys._host(p, 16).view(np.int64).reshape(1, 16)).to(dev)
             for p in points]
    with torch.cuda.device(dev):
        _fail_unless(ceremony.g2_subgroup_check(torch.cat(parts).contiguous()) < 0, "g2 subgroup")


def _first_failure(order, verdicts: dict, flags: dict):
    """the first check of `order` that failed: pairings from `verdicts`, byte equalities from `flags`"""
    for check in order:
        _fail_unless(verdicts[check] if check in verdicts else flags[check], check)


# ---------------------------------------------------------------------------------------------------------------
# phase 2
def _to_dev(rec, device):
    import torch

    a = keys._host(rec, np.asarray(rec).size)
    return torch.from_numpy(a.view(np.int64).reshape(1, -1).copy()).to(device)


def contribute_mpc_parameters(mpc, delta: int = None):
    """MPCParameters::contribute (parameters.rs:414-522): the key pair (keys.mpc_keypair), every point of l and h by delta^-1 and the two
    delta elements by delta (ceremony.contribute_parameters), the public key appended, its hash.  Returns (the new parameters, hash64);
    `mpc` is not modified.  delta: the private key, from the `secrets` module when None."""
    import torch

    dev = mpc["params"]["h"].device
    pub, delta = keys.mpc_keypair(mpc, delta)
    params = ceremony.contribute_parameters(mpc["params"], delta)
    pk = {k: _to_dev(pub[k], dev) for k in ("delta_after", "s", "s_delta", "r_delta")}
    pk["transcript"] = torch.frombuffer(bytearray(pub["transcript"]), dtype=torch.uint8).to(dev)
    out = {"params": params, "cs_hash": mpc["cs_hash"], "contributions": list(mpc["contributions"]) + [pk]}
    return out, keys.mpc_public_key_hash(pub)


_UNCHANGED = (("a", lambda p: p["a"]), ("b_g1", lambda p: p["b_g1"]), ("b_g2", lambda p: p["b_g2"]), ("alpha_g1", lambda p: p["vk"]["alpha_g1"]),
              ("beta_g1", lambda p: p["vk"]["beta_g1"]), ("beta_g2", lambda p: p["vk"]["beta_g2"]), ("gamma_g2", lambda p: p["vk"]["gamma_g2"]),
              ("ic", lambda p: p["vk"]["ic"]))


def _unchanged_parts(before, after):
    """parameters.rs:538-579 / 741-782: lengths of h and l, then everything a contribution must not touch"""
    _fail_unless(before["params"]["h"].shape[0] == after["params"]["h"].shape[0], "h length")
    _fail_unless(before["params"]["l"].shape[0] == after["params"]["l"].shape[0], "l length")
    for name, get in _UNCHANGED:
        _fail_unless(_same(get(before["params"]), get(after["params"])), name)
    _fail_unless(_bytes(before["cs_hash"]) == _bytes(after["cs_hash"]), "cs_hash")


def _same_public_key(a, b) -> bool:
    return keys.mpc_public_key_bytes(a) == keys.mpc_public_key_bytes(b)


def verify_contribution(before, after, key: bytes = None, check_g2_subgroup: bool = True) -> bytes:
    """verify_contribution (parameters.rs:726-854) over two dicts as ceremony.read_mpc_parameters returns them -> the contribution's hash.
    Five same_ratio checks, one pairing launch."""
    nb = len(before["contributions"])
    _fail_unless(len(after["contributions"]) == nb + 1, "contribution count")
    _fail_unless(all(_same_public_key(x, y) for x, y in zip(before["contributions"], after["contributions"])), "previous contributions")
    _unchanged_parts(before, after)
    pubkey = after["contributions"][-1]
    h = keys.mpc_transcript(_bytes(before["cs_hash"]), before["contributions"], pubkey["s"], pubkey["s_delta"])
    _fail_unless(_bytes(pubkey["transcript"]) == h, "transcript")
    bp, ap = before["params"], after["params"]
    _subgroup([pubkey["r_delta"], ap["vk"]["delta_g2"], bp["vk"]["delta_g2"]], check_g2_subgroup)
    r = keys.hash_to_g2(h)
    ex = _Exponents(key)
    ratios = _Ratios(ap["h"].device)
    ratios.add("signature of knowledge", (pubkey["s"], pubkey["s_delta"]), (r, pubkey["r_delta"]))      # same_ratio((r, r_delta), (s, s_delta))
    ratios.add("delta_g1 change", (bp["vk"]["delta_g1"], pubkey["delta_after"]), (r, pubkey["r_delta"]))
    ratios.add("delta_g2", (ceremony.G1_ONE_RAW, pubkey["delta_after"]), (ceremony.G2_ONE_RAW, ap["vk"]["delta_g2"]))
    ratios.add("h", _merged(bp["h"], ap["h"], ex), (ap["vk"]["delta_g2"], bp["vk"]["delta_g2"]))     # reversed for the inverse
    ratios.add("l", _merged(bp["l"], ap["l"], ex), (ap["vk"]["delta_g2"], bp["vk"]["delta_g2"]))
    flags = {"delta_after": np.array_equal(keys._host(pubkey["delta_after"], 8), keys._host(ap["vk"]["delta_g1"], 8))}
    _first_failure(("signature of knowledge", "delta_g1 change", "delta_after", "delta_g2", "h", "l"), ratios.run(), flags)
    return keys.mpc_public_key_hash(pubkey)


def verify_mpc_parameters(mpc, circuit, should_filter_points_at_infinity: bool, radix, key: bytes = None, check_g2_subgroup: bool = True):
    """MPCParameters::verify (parameters.rs:529-659): the parameters are those circom.mpc_parameters_new derives from `circuit` and `radix`,
    transformed by the recorded contributions -> the list of the contributions' hashes.  2 k + 3 same_ratio checks, one pairing launch."""
    initial = circom.mpc_parameters_new(circuit, should_filter_points_at_infinity, radix)
    _unchanged_parts(initial, mpc)
    ip, p = initial["params"], mpc["params"]
    contributions = mpc["contributions"]
    _subgroup([pk["r_delta"] for pk in contributions] + [p["vk"]["delta_g2"]], check_g2_subgroup)
    ex = _Exponents(key)
    ratios = _Ratios(p["h"].device)
    sink = hashlib.blake2b(_bytes(initial["cs_hash"]), digest_size=64)
    current_delta, order, flags, result = ceremony.G1_ONE_RAW, [], {}, []
    for i, pk in enumerate(contributions):
        ours = sink.copy()
        ours.update(keys.point_to_uncompressed(keys._host(pk["s"], 8)))
        ours.update(keys.point_to_uncompressed(keys._host(pk["s_delta"], 8)))
        sink.update(keys.mpc_public_key_bytes(pk))
        h = ours.digest()
        r = keys.hash_to_g2(h)
        names = [f"{c} of contribution {i}" for c in ("transcript", "signature of knowledge", "delta_g1 change")]
        flags[names[0]] = _bytes(pk["transcript"]) == h
        ratios.add(names[1], (pk["s"], pk["s_delta"]), (r, pk["r_delta"]))
        ratios.add(names[2], (current_delta, pk["delta_after"]), (r, pk["r_delta"]))
        order += names
        current_delta = pk["delta_after"]
        result.append(keys.mpc_public_key_hash(pk))
    flags["delta_after"] = np.array_equal(keys._host(current_delta, 8), keys._host(p["vk"]["delta_g1"], 8))
    ratios.add("delta_g2", (ceremony.G1_ONE_RAW, current_delta), (ceremony.G2_ONE_RAW, p["vk"]["delta_g2"]))
    ratios.add("h", _merged(ip["h"], p["h"], ex), (p["vk"]["delta_g2"], ceremony.G2_ONE_RAW))
    ratios.add("l", _merged(ip["l"], p["l"], ex), (p["vk"]["delta_g2"], ceremony.G2_ONE_RAW))
    _first_failure(order + ["delta_after", "delta_g2", "h", "l"], ratios.run(), flags)
    return result


# ---------------------------------------------------------------------------------------------------------------
# powers of tau
def _file_tensor(data, device=None):
    import torch

    if hasattr(data, "is_cuda"):
        return data
    device = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return torch.frombuffer(bytearray(bytes(data)), dtype=torch.uint8).to(device)


def contribute_response(challenge_bytes, power: int, tau: int = None, alpha: int = None, beta: int = None, device=None, checked: bool = True):
    """compute_constrained: the hash of the challenge file, a key pair bound to it (keys.keypair), ceremony.contribute_accumulator, and
    the response file -- the challenge's hash, the COMPRESSED accumulator, the public key -- as a uint8 device tensor.  The secrets come
    from the `secrets` module when not given.  Returns (response, public key)."""
    import torch

    data = _file_tensor(challenge_bytes, device)
    digest = ceremony.calculate_hash(data)
    acc = ceremony.read_accumulator(data, power, compressed=False, checked=checked)
    pub, priv = keys.keypair(digest, tau, alpha, beta)
    out = ceremony.contribute_accumulator(acc, priv["tau"], priv["alpha"], priv["beta"])
    out["hash"] = torch.frombuffer(bytearray(digest), dtype=torch.uint8).to(data.device)
    body = ceremony.write_accumulator(out, compressed=True)
    tail = torch.frombuffer(bytearray(keys.write_public_key(pub)), dtype=torch.uint8).to(data.device)
    return torch.cat([body, tail]), pub


def read_response(response_bytes, power: int, device=None, checked: bool = True):
    """a response file -> (the accumulator as ceremony.read_accumulator returns it, the public key behind it)"""
    data = _file_tensor(response_bytes, device)
    _, total = ceremony.accumulator_layout(power, True)
    if data.numel() != total + keys.PUBLIC_KEY_SIZE:
        raise ValueError(f"a response of power {power} has {total + keys.PUBLIC_KEY_SIZE} bytes")
    return ceremony.read_accumulator(data[:total], power, compressed=True, checked=checked), keys.read_public_key(_bytes(data[total:]))


def next_challenge(response_bytes, power: int, device=None):
    """What verify_transform_constrained writes after it has accepted a response: the UNCOMPRESSED accumulator headed by the hash of the
    response file -- the next contributor's challenge, as a uint8 device tensor."""
    import torch

    data = _file_tensor(response_bytes, device)
    acc, _ = read_response(data, power, checked=False)
    acc["hash"] = torch.frombuffer(bytearray(ceremony.calculate_hash(data)), dtype=torch.uint8).to(data.device)
    return ceremony.write_accumulator(acc, compressed=False)


_ACC_VECTORS = ("tau_g1", "tau_g2", "alpha_g1", "beta_g1", "beta_g2")


def _decide_transform(device, pk, digest: bytes, before, after, powers):
    """The eleven same_ratio checks and the two byte equalities of verify_transform in ONE pairing launch, read in the reference's order.
    before / after: {vector: its first records} (two of tau_g1 and tau_g2 are used, one of the others; device tensors or host records);
    powers: {vector: power_pairs of the whole vector as a pair of affine host records}.  Shared by the in-memory flow below and the
    file-to-file flow of stream.py, which gets `powers` from chunked sums."""
    g2_s = {name: keys.compute_g2_s(digest, pk[f"{name}_g1_s"], pk[f"{name}_g1_s_{name}"], i) for i, name in enumerate(("tau", "alpha", "beta"))}
    ratios = _Ratios(device)
    for name in ("tau", "alpha", "beta"):
        ratios.add(f"{name} proof of knowledge", (pk[f"{name}_g1_s"], pk[f"{name}_g1_s_{name}"]), (g2_s[name], pk[f"{name}_g2"]))
    ratios.add("tau change", (before["tau_g1"][1], after["tau_g1"][1]), (g2_s["tau"], pk["tau_g2"]))
    ratios.add("alpha change", (before["alpha_g1"][0], after["alpha_g1"][0]), (g2_s["alpha"], pk["alpha_g2"]))
    ratios.add("beta change", (before["beta_g1"][0], after["beta_g1"][0]), (g2_s["beta"], pk["beta_g2"]))
    ratios.add("beta_g2 change", (before["beta_g1"][0], after["beta_g1"][0]), (before["beta_g2"][0], after["beta_g2"][0]))
    tau_g1_pair, tau_g2_pair = (after["tau_g1"][0], after["tau_g1"][1]), (after["tau_g2"][0], after["tau_g2"][1])
    ratios.add("tau_g1 powers", powers["tau_g1"], tau_g2_pair)
    ratios.add_g2_first("tau_g2 powers", powers["tau_g2"], tau_g1_pair)
    ratios.add("alpha_g1 powers", powers["alpha_g1"], tau_g2_pair)
    ratios.add("beta_g1 powers", powers["beta_g1"], tau_g2_pair)
    flags = {"tau_g1[0]": np.array_equal(keys._host(after["tau_g1"][0], 8), ceremony.G1_ONE_RAW),
             "tau_g2[0]": np.array_equal(keys._host(after["tau_g2"][0], 16), ceremony.G2_ONE_RAW)}
    _first_failure(("tau proof of knowledge", "alpha proof of knowledge", "beta proof of knowledge", "tau_g1[0]", "tau_g2[0]", "tau change",
                    "alpha change", "beta change", "beta_g2 change", "tau_g1 powers", "tau_g2 powers", "alpha_g1 powers", "beta_g1 powers"),
                   ratios.run(), flags)


def verify_transform(before, after, public_key, digest: bytes, key: bytes = None, check_g2_subgroup: bool = True) -> bool:
    """verify_transform (batched_accumulator.rs:182-272): `after` is `before` (two dicts as ceremony.read_accumulator returns them)
    transformed by the holder of `public_key` (keys.read_public_key), for the 64-byte transcript `digest` (the hash of the challenge
    file).  True, or VerificationError.  Eleven same_ratio checks, one pairing launch."""
    digest = bytes(digest)
    if len(digest) != 64:
        raise ValueError("the transcript digest has 64 bytes")
    for name in _ACC_VECTORS:
        _fail_unless(before[name].shape == after[name].shape, f"{name} length")
    _fail_unless(after["tau_g1"].shape[0] >= 2 and after["tau_g2"].shape[0] >= 2, "tau powers length")
    pk = public_key
    _subgroup([after["tau_g2"], after["beta_g2"], before["beta_g2"], pk["tau_g2"], pk["alpha_g2"], pk["beta_g2"]], check_g2_subgroup)
    ex = _Exponents(key)
    powers = {name: _powers(after[name], ex) for name in ("tau_g1", "tau_g2", "alpha_g1", "beta_g1")}
    _decide_transform(after["tau_g1"].device, pk, digest, {"tau_g1": before["tau_g1"][:2], "alpha_g1": before["alpha_g1"][:1],
                      "beta_g1": before["beta_g1"][:1], "beta_g2": before["beta_g2"][:1]},
                      {name: after[name][:2] for name in _ACC_VECTORS}, powers)
    return True
