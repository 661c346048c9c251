#!/usr/bin/env python3
"""Generates tests/golden/bellman_patch_preimage.json: for every hunk of integration/bellman_mi355zk.patch, the sha256 of the
lines it replaces or keeps as context, as they stand in the reference's bellman/ tree (read from that tree, not from the patch),
with the hunk's line range and each file's line count.  Digests only: no text of the reference is stored.
tests/test_integration_patch.py checks the patch's pre-image against these digests and applies the patch to files rebuilt
from it, so that check needs nothing outside this repository.
Run:  python tests/golden/gen_bellman_preimage.py <the reference's bellman/ directory>   (rewrites the JSON file)
"""
import hashlib
import json
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
PATCH = os.path.join(os.path.dirname(os.path.dirname(HERE)), "integration", "bellman_mi355zk.patch")


def old_ranges(patch_text):
    """{relative path: [(first line, count), ...]}: the pre-image side of every hunk (files the patch creates have none)"""
    ranges, cur = {}, None
    for ln in patch_text.splitlines():
        if ln.startswith("--- a/"):
            cur = ln[len("--- a/"):].split("\t")[0]
        m = re.match(r"@@ -(\d+)(?:,(\d+))? \+\d+(?:,\d+)? @@", ln)
        if m and cur is not None:
            first, count = int(m.group(1)), int(m.group(2) if m.group(2) is not None else 1)
            if count:
                ranges.setdefault(cur, []).append((first, count))
    return ranges


def digest(lines):
    return hashlib.sha256("".join(ln + "\n" for ln in lines).encode()).hexdigest()


def main(bellman):
    files = {}
    for rel, hunks in sorted(old_ranges(open(PATCH).read()).items()):
        lines = open(os.path.join(bellman, rel)).read().split("\n")
        if lines[-1] == "":   # (a final newline ends the last line; src/domain.rs has none)
            lines = lines[:-1]
        files[rel] = {"lines": len(lines), "hunks": [[first, count, digest(lines[first - 1:first - 1 + count])] for first, count in hunks]}
    doc = {"what": "sha256 of the pre-image lines of each hunk of integration/bellman_mi355zk.patch in the reference's bellman/ tree "
                   "([first line (1-based), line count, sha256 of those lines joined with newlines]) and each file's line count",
           "files": files}
    with open(os.path.join(HERE, "bellman_patch_preimage.json"), "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit("usage: gen_bellman_preimage.py <the reference's bellman/ directory>")
    main(sys.argv[1])
