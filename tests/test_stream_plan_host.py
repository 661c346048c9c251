"""The chunk plan of phase2-bn254_amd/stream.py (the reference's: batched_accumulator.rs:394-397, 465-475) as pure host arithmetic: every
index of every vector is owned by exactly one chunk, the chunks a verification reads overlap their successor by exactly one record and
never leave their range, the pair across the two ranges of tau_g1 is covered, and the byte offsets are those of accumulator_layout."""
import pytest

POWERS = (1, 2, 3, 4, 5, 6)
BATCH_SIZES = (2, 3, 5, 16, 1000)
SIZE = {(1, False): 64, (1, True): 32, (2, False): 128, (2, True): 64}


def _counts(power):
    n = 1 << power
    return {"tau_g1": 2 * n - 1, "tau_g2": n, "alpha_g1": n, "beta_g1": n, "beta_g2": 1}


@pytest.mark.parametrize("power", POWERS)
@pytest.mark.parametrize("batch_size", BATCH_SIZES)
def test_every_index_is_owned_exactly_once(zk, power, batch_size):
    owned = {name: [0] * cnt for name, cnt in _counts(power).items()}
    for b in zk.batches(power, batch_size):
        assert b.count >= 0 and b.count <= batch_size
        for i in range(b.start, b.start + b.count):
            owned[b.vector][i] += 1
    assert all(set(v) == {1} for v in owned.values())


@pytest.mark.parametrize("power", POWERS)
@pytest.mark.parametrize("batch_size", BATCH_SIZES)
def test_verification_chunks_overlap_by_one_record_inside_their_range(zk, power, batch_size):
    n = 1 << power
    plan = zk.batches(power, batch_size)
    for name, cnt in _counts(power).items():
        for lo, hi in ((0, min(n, cnt)), (n, cnt)):
            chunks = [b for b in plan if b.vector == name and b.count and lo <= b.start < hi]
            if hi <= lo:
                assert not chunks
                continue
            assert chunks[0].start == lo
            for b, nxt in zip(chunks, chunks[1:]):
                assert b.verify_count == b.count + 1 and b.start + b.verify_count == nxt.start + 1   # shares exactly its last record
            last = chunks[-1]
            assert last.verify_count == last.count and last.start + last.verify_count == hi          # never past the range's end
            assert all(b.verify_count <= batch_size + 1 for b in chunks)


@pytest.mark.parametrize("power", POWERS)
@pytest.mark.parametrize("batch_size", BATCH_SIZES)
def test_every_pair_of_neighbours_lies_in_one_chunk(zk, power, batch_size):
    """what makes the chunked power_pairs sums the whole vector's: the junction 2^p - 1 | 2^p of tau_g1 included, each pair exactly once"""
    n = 1 << power
    plan = zk.batches(power, batch_size)
    for name, cnt in _counts(power).items():
        pairs = [0] * max(cnt - 1, 0)
        for b in plan:
            if b.vector == name:
                assert b.verify_count >= 1 and b.start + b.verify_count <= cnt
                for i in range(b.start, b.start + b.verify_count - 1):
                    pairs[i] += 1
        assert all(p == 1 for p in pairs), (name, pairs)
    junction = [b for b in plan if b.vector == "tau_g1" and b.start <= n - 1 and b.start + b.verify_count >= n + 1]
    assert len(junction) == 1
    assert junction[0].count == 0 and junction[0].verify_count == 2      # its own pair: it owns nothing


@pytest.mark.parametrize("power", POWERS)
@pytest.mark.parametrize("batch_size", BATCH_SIZES)
def test_byte_offsets_are_the_layouts(zk, power, batch_size):
    plan = zk.batches(power, batch_size)
    for compressed in (False, True):
        layout, total = zk.ceremony.accumulator_layout(power, compressed)
        at = {name: (g, off) for name, g, _, off in layout}
        end = 0
        for b in plan:
            g, off = at[b.vector]
            assert b.group == g
            got = b.compressed_offset if compressed else b.uncompressed_offset
            assert got == off + b.start * SIZE[(g, compressed)]
            end = max(end, got + max(b.count, b.verify_count) * SIZE[(g, compressed)])
        assert end == total                                                  # the plan reaches the last byte of the body and no further
        if compressed:
            assert zk.stream.response_size(power) == total + zk.keys.PUBLIC_KEY_SIZE
        else:
            assert zk.stream.challenge_size(power) == total


@pytest.mark.parametrize("batch_size", (0, 1, -3))
def test_a_batch_size_below_two_is_refused(zk, batch_size):
    with pytest.raises(ValueError):
        zk.batches(4, batch_size)


def test_hash_of_a_file_is_blake2b_of_its_bytes(zk, tmp_path, monkeypatch):
    import hashlib

    blob = bytes(range(256)) * 37 + b"tail"
    path = tmp_path / "blob"
    path.write_bytes(blob)
    want = hashlib.blake2b(blob, digest_size=64).digest()
    assert zk.calculate_hash_file(path) == want
    monkeypatch.setattr(zk.stream, "_HASH_SLICE", 1000)                      # several slices, a ragged last one
    assert zk.calculate_hash_file(path) == want
    (tmp_path / "empty").write_bytes(b"")
    assert zk.calculate_hash_file(tmp_path / "empty") == zk.ceremony.blank_hash()


def test_new_constrained_writes_generators_behind_the_blank_hash(zk, tmp_path):
    """host-only: the file's size, head and records (the byte comparison with the in-memory flow is tests/test_gpu_stream.py's)"""
    power = 3
    digests = set()
    for batch_size in (2, 5, 1000):
        path = tmp_path / f"challenge{batch_size}"
        digest = zk.new_constrained(path, power, batch_size)
        data = path.read_bytes()
        assert len(data) == zk.stream.challenge_size(power) and digest == zk.calculate_hash_file(path)
        assert data[:64] == zk.ceremony.blank_hash()
        g1, g2 = zk.keys.point_to_uncompressed(zk.ceremony.G1_ONE_RAW), zk.keys.point_to_uncompressed(zk.ceremony.G2_ONE_RAW)
        assert data[64:] == g1 * 15 + g2 * 8 + g1 * 8 + g1 * 8 + g2
        digests.add(digest)
    assert len(digests) == 1
