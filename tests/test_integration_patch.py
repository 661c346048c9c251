"""The Rust side of the boundary, machine-checked as far as an image without rustc allows:
  - integration/mi355zk.rs's `extern "C"` block is the one tools/gen_rust_ffi.py derives from include/mi355zk.h, and -- parsed back
    independently -- every item has the name, the argument count and the pointer / integer shape of its C prototype;
  - the symbols the hand-written shim code calls exist in that block;
  - integration/bellman_mi355zk.patch carries exactly that file as bellman/src/mi355zk.rs and applies (`patch --dry-run -p1`) to the
    reference's bellman/ tree (multiexp.rs:330-355, source.rs:21-34,72-118, domain.rs:263-272): every hunk's pre-image is the text the
    reference holds at that place (sha256 digests taken from the reference tree: tests/golden/bellman_patch_preimage.json, written by
    tests/golden/gen_bellman_preimage.py), and the patch applies to files rebuilt from those pre-images."""
import hashlib
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import gen_rust_ffi as gen  # noqa: E402

RS = os.path.join(ROOT, "integration", "mi355zk.rs")
PATCH = os.path.join(ROOT, "integration", "bellman_mi355zk.patch")
PREIMAGE = os.path.join(ROOT, "tests", "golden", "bellman_patch_preimage.json")


def _rust_items():
    """{name: ([argument types], return type or None)} of the extern block, parsed from the Rust text (not from the generator)"""
    src = open(RS).read()
    m = re.search(r'extern "C" \{(.*?)\n\}', src, flags=re.S)
    assert m, "no extern block"
    items = {}
    for fm in re.finditer(r"pub fn (\w+)\((.*?)\)( -> ([^;]+))?;", m.group(1), flags=re.S):
        args = re.sub(r"/\*.*?\*/", "", fm.group(2))
        types = [a.split(":", 1)[1].strip() for a in args.split(",") if a.strip()]
        items[fm.group(1)] = (types, fm.group(4).strip() if fm.group(4) else None)
    return items


def test_extern_block_is_generated_from_the_header():
    assert gen.main.__module__ == "gen_rust_ffi"
    src = open(RS).read()
    i, j = src.index(gen.BEGIN), src.index(gen.END) + len(gen.END)
    assert src[i:j] == gen.block(), "integration/mi355zk.rs is stale: run tools/gen_rust_ffi.py"


def test_every_extern_item_matches_its_c_prototype():
    items = _rust_items()
    protos = {name: (ret, params) for ret, name, params in gen.prototypes()}
    public = [n for n in protos if not n.startswith(("mi355zk_selftest_", "mi355zk_ubench_"))]
    assert sorted(items) == sorted(public)
    for name, (types, ret) in items.items():
        c_ret, c_params = protos[name]
        assert len(types) == len(c_params), name
        assert (ret is None) == (c_ret == "void"), name
        for rt, (ct, _) in zip(types, c_params):
            c_is_ptr = "*" in ct or "[" in ct
            assert rt.startswith(("*const", "*mut")) == c_is_ptr, (name, rt, ct)
            if c_is_ptr:
                assert rt.startswith("*const") == ct.startswith("const ") or ct.replace(" ", "") == "void*const*", (name, rt, ct)
            else:
                assert rt == {"int": "c_int", "size_t": "usize", "uint32_t": "u32", "uint64_t": "u64", "long long": "c_longlong"}[ct], (name, rt, ct)


def test_the_shim_only_calls_declared_symbols():
    src = open(RS).read()
    body = src[src.index(gen.END):]
    called = set(re.findall(r"\b(mi355zk_\w+)\s*\(", body))
    assert {"mi355zk_bn254_g1_msm", "mi355zk_bn254_g2_msm", "mi355zk_bn254_fr_ntt", "mi355zk_bn254_g1_to_affine", "mi355zk_bn254_g2_to_affine"} <= called
    assert called <= set(_rust_items())


def test_the_patch_carries_this_file():
    patch = open(PATCH).read()
    m = re.search(r"^\+\+\+ b/src/mi355zk\.rs\n@@ -0,0 \+1,(\d+) @@\n((?:\+.*\n)+)", patch, flags=re.M)
    assert m, "the patch does not add src/mi355zk.rs"
    added = "".join(ln[1:] + "\n" for ln in m.group(2).splitlines())
    assert added == open(RS).read(), "integration/bellman_mi355zk.patch is stale: run integration/make_patch.py"
    for f in ("Cargo.toml", "src/lib.rs", "src/source.rs", "src/multiexp.rs", "src/domain.rs"):
        assert "+++ b/%s\n" % f in patch, f
    assert "try_multiexp::<Q, D, G, S>" in patch and "try_best_fft::<E, T>" in patch


def _preimages():
    """{relative path: [(first line, [pre-image lines]), ...]} of the patch's hunks (context and removed lines), from the patch itself"""
    hunks, cur, lines = {}, None, iter(open(PATCH).read().splitlines())
    for ln in lines:
        if ln.startswith("--- a/"):
            cur = ln[len("--- a/"):].split("\t")[0]
        m = re.match(r"@@ -(\d+)(?:,(\d+))? \+\d+(?:,(\d+))? @@", ln)
        if not m:
            continue
        old, new, pre = int(m.group(2) or 1), int(m.group(3) or 1), []
        while old or new:
            body = next(lines)
            if body.startswith("\\"):
                continue
            tag, text = body[:1], body[1:]
            if tag in (" ", "-"):
                pre.append(text)
                old -= 1
            if tag in (" ", "+"):
                new -= 1
        if pre:
            hunks.setdefault(cur, []).append((int(m.group(1)), pre))
    return hunks


def _digest(lines):
    """as tests/golden/gen_bellman_preimage.py takes it from the reference tree"""
    return hashlib.sha256("".join(ln + "\n" for ln in lines).encode()).hexdigest()


def test_the_patch_preimage_is_the_reference_text():
    """Each hunk replaces or keeps exactly the lines the reference's bellman/ holds at its line range, so `patch` applies it in place, no fuzz."""
    want = json.load(open(PREIMAGE))["files"]
    got = _preimages()
    assert sorted(got) == sorted(want)
    for rel, hunks in got.items():
        assert [[first, len(pre), _digest(pre)] for first, pre in hunks] == want[rel]["hunks"], rel


@pytest.mark.skipif(shutil.which("patch") is None, reason="needs patch(1)")
def test_the_patch_applies_to_the_reference_tree(tmp_path):
    # the reference's files as far as the patch reads them: every hunk's pre-image at its line (the digests above tie it to the reference
    # text), a placeholder on every other line, each file its reference length
    work = tmp_path / "bellman"
    want = json.load(open(PREIMAGE))["files"]
    for rel, hunks in _preimages().items():
        lines = ["// reference line %d (not stored)" % (i + 1) for i in range(want[rel]["lines"])]
        for first, pre in hunks:
            lines[first - 1:first - 1 + len(pre)] = pre
        (work / rel).parent.mkdir(parents=True, exist_ok=True)
        (work / rel).write_text("".join(ln + "\n" for ln in lines))
    r = subprocess.run(["patch", "--dry-run", "-p1", "-i", PATCH], cwd=work, capture_output=True, text=True)
    assert r.returncode == 0 and "FAILED" not in r.stdout and "fuzz" not in r.stdout, r.stdout + r.stderr
    r = subprocess.run(["patch", "-p1", "-i", PATCH], cwd=work, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert (work / "src" / "mi355zk.rs").read_text() == open(RS).read()
    src = (work / "src" / "multiexp.rs").read_text()
    # the early return sits between the query-size assertion and the reference's own call (multiexp.rs:347-354)
    assert src.index("assert!(query_size == exponents.len());") < src.index("crate::mi355zk::try_multiexp") < src.index("multiexp_inner_impl(pool, bases, density_map, exponents, 0, c, true)")
