#!/usr/bin/env python3
"""Writes tests/golden/pairing_golden.json from the big-int model (tests/pairing_model.py): GT values in the library's 384-byte format
(48 u64 words, hex), which the host product and the kernels must reproduce byte for byte.

  e_g1_g2   e(G1, G2) of the generators
  pairs     e(a G1, b G2) for six fixed (a, b): small, full width, a = r - 1
  jeff1     the two pairs of the EIP-197 "jeff1" vector (tests/test_oracle_public_vectors.py: PAIRING_JEFF1), each pair's own GT value;
            their product is one

Run from the repository root:  python tests/golden/gen_pairing_golden.py   (a few seconds)
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import bn254_model as M  # noqa: E402
import pairing_model as P  # noqa: E402

R = M.R_ORDER
PAIRS = [(2, 1), (3, 5), (R - 1, 1), (R - 1, R - 1),
         (0x1B7E4D3C2A190807F6E5D4C3B2A1908F7E6D5C4B3A29180706F5E4D3C2B1A09 % R, 0x2468ACE013579BDF02468ACE13579BDF2468ACE013579BDF02468ACE13579BD % R),
         (0x2F0E1D2C3B4A59687796A5B4C3D2E1F00F1E2D3C4B5A69788796A5B4C3D2E1F % R, 7)]


def jeff1_points():
    """[(G1 point, G2 point)] of the vector: x || y, then x.c1 || x.c0 || y.c1 || y.c0, 32-byte big-endian words"""
    from test_oracle_public_vectors import PAIRING_JEFF1

    w = [int(PAIRING_JEFF1[i:i + 64], 16) for i in range(0, len(PAIRING_JEFF1), 64)]
    return [((w[6 * k], w[6 * k + 1]), ((w[6 * k + 3], w[6 * k + 2]), (w[6 * k + 5], w[6 * k + 4]))) for k in range(2)]


def hexwords(words):
    return ["%016x" % v for v in words]


def main():
    out = {"e_g1_g2": hexwords(P.gt_to_words(P.pairing(M.G1_GEN, M.G2_GEN))), "pairs": [], "jeff1": []}
    for a, b in PAIRS:
        gt = P.pairing(M.ec_mul(M.FQ_OPS, M.G1_GEN, a), M.ec_mul(M.FQ2_OPS, M.G2_GEN, b))
        out["pairs"].append({"a": "%x" % a, "b": "%x" % b, "gt": hexwords(P.gt_to_words(gt))})
    for p, q in jeff1_points():
        out["jeff1"].append({"g1": hexwords(M.g1_affine_to_raw(p)), "g2": hexwords(M.g2_affine_to_raw(q)), "gt": hexwords(P.gt_to_words(P.pairing(p, q)))})
    with open(os.path.join(HERE, "pairing_golden.json"), "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
