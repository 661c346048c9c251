#!/usr/bin/env python3
"""Writes tests/golden/hash_to_g2.json from the big-int model (tests/ceremony_model.py: its own ChaCha20, bn254_model's affine curve code):
hash_to_g2 (powersoftau/src/utils.rs:31-45) of fixed digests, each result as the 16 u64 words (hex) of a raw affine G2 record, which
phase2-bn254_amd/keys.py must reproduce word for word.  The digests: the reference's own test input (utils.rs:56-72: the bytes 1 .. 32),
all zero, all 0xff, and BLAKE2b-512 of the empty string (the hash of a fresh challenge).

Run from the repository root:  python tests/golden/gen_hash_to_g2_golden.py   (under a second)
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import bn254_model as M  # noqa: E402
import ceremony_model as CM  # noqa: E402

DIGESTS = [bytes(range(1, 33)), bytes(32), bytes([0xFF]) * 32, hashlib.blake2b(b"", digest_size=64).digest()]


def main():
    out = {"cases": [{"digest": d.hex(), "g2": ["%016x" % v for v in M.g2_affine_to_raw(CM.hash_to_g2(d))]} for d in DIGESTS]}
    with open(os.path.join(HERE, "hash_to_g2.json"), "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
