"""Strided affine records, host side (no GPU): the new entry points are exported and bound, every argument rule of the strided layout
returns 3 before any device work, the Rust shim takes the strided path, and the C++ program over a bellman-like record type compiles
against the header (tests/cpp/test_strided_records.cpp; it runs on the GPU in tests/test_gpu_msm_strided.py)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS = os.path.join(ROOT, "integration", "mi355zk.rs")
HDR = os.path.join(ROOT, "include", "mi355zk.h")
NEW = ["mi355zk_bn254_g1_msm_strided", "mi355zk_bn254_g2_msm_strided", "mi355zk_bases_cache_pin_strided",
       "mi355zk_bn254_g1_records_pack_dev", "mi355zk_bn254_g2_records_pack_dev"]


def build_cpp():
    """g++ tests/cpp/test_strided_records.cpp -> build/test_strided_records (links libmi355zk.so and the oracle)"""
    os.makedirs(os.path.join(ROOT, "build"), exist_ok=True)
    exe = os.path.join(ROOT, "build", "test_strided_records")
    import torch  # the binary must resolve libamdhip64 the same way the python process does

    cmd = ["g++", "-std=c++17", "-O2", "-Wall", os.path.join(ROOT, "tests", "cpp", "test_strided_records.cpp"), "-o", exe,
           "-L" + os.path.join(ROOT, "phase2-bn254_amd"), "-lmi355zk", "-L" + os.path.join(ROOT, "oracle", "_build"), "-loracle",
           "-Wl,-rpath," + os.path.join(ROOT, "phase2-bn254_amd"), "-Wl,-rpath," + os.path.join(ROOT, "oracle", "_build"), "-lpthread"]
    subprocess.check_call(cmd)
    return exe


@pytest.fixture(scope="module")
def lib():
    import phase2_bn254_amd as zk

    return zk.lib.load()


def test_new_symbols_are_exported_and_bound(lib):
    import phase2_bn254_amd as zk

    text = re.sub(r"/\*.*?\*/", "", open(HDR).read(), flags=re.S)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name) and name in zk.lib.SIGNATURES, name
    assert lib.mi355zk_abi_version() == zk.lib.ABI_VERSION == 7


NF = (1 << 64) - 1
# (group, stride, x_off, y_off, inf_off) that the library must refuse
BAD = [
    (1, 70, 0, 32, 64),        # stride not a multiple of 4
    (1, 4100, 0, 32, 64),      # stride > 4096
    (1, 0, 0, 32, NF),         # stride 0
    (1, 60, 0, 28, NF),        # stride too small for two coordinates
    (1, 72, 2, 36, 70),        # x_off misaligned
    (1, 72, 0, 34, 70),        # y_off misaligned
    (1, 72, 0, 16, 64),        # x and y overlap
    (1, 72, 16, 0, 64),        # y and x overlap
    (1, 72, 0, 44, 40),        # y runs past the record
    (1, 72, 0, 32, 10),        # inf_off inside x
    (1, 72, 0, 32, 40),        # inf_off inside y
    (1, 72, 0, 32, 72),        # inf_off >= stride
    (2, 136, 0, 32, 128),      # G2: coordinates of 64 bytes overlap
    (2, 136, 0, 64, 100),      # G2: inf_off inside y
    (2, 120, 0, 64, NF),       # G2: stride too small
    (2, 136, 4, 68, 136),      # G2: inf_off >= stride
]


@pytest.mark.parametrize("group, stride, x_off, y_off, inf_off", BAD)
def test_bad_layouts_return_3_without_a_device(lib, group, stride, x_off, y_off, inf_off):
    buf = np.zeros(64 * 4096, np.uint8)
    sc = np.zeros((4, 4), np.uint64)
    out = np.zeros(24, np.uint64)
    p, s, o = buf.ctypes.data_as(C.c_void_p), sc.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    msm = lib.mi355zk_bn254_g1_msm_strided if group == 1 else lib.mi355zk_bn254_g2_msm_strided
    pack = lib.mi355zk_bn254_g1_records_pack_dev if group == 1 else lib.mi355zk_bn254_g2_records_pack_dev
    assert msm(p, 4, stride, x_off, y_off, inf_off, 0, s, 4, None, 0, o) == 3
    assert lib.mi355zk_bases_cache_pin_strided(p, 4, stride, x_off, y_off, inf_off, group, 0) == 3
    assert pack(p, 4, stride, x_off, y_off, inf_off, o, None) == 3


def test_other_argument_rules_return_3(lib):
    buf = np.zeros(72 * 8, np.uint8)
    p = buf.ctypes.data_as(C.c_void_p)
    for group in (0, 3, -1):
        assert lib.mi355zk_bases_cache_pin_strided(p, 8, 72, 0, 32, 64, group, 0) == 3
    assert lib.mi355zk_bases_cache_pin_strided(p, 8, 72, 0, 32, 64, 1, 2) == 3         # unknown flag bit
    assert lib.mi355zk_bases_cache_pin_strided(None, 8, 72, 0, 32, 64, 1, 0) == 3      # NULL
    assert lib.mi355zk_bases_cache_pin_strided(p, 0, 72, 0, 32, 64, 1, 0) == 3         # empty
    out = np.zeros(12, np.uint64)
    o = out.ctypes.data_as(C.c_void_p)
    assert lib.mi355zk_bn254_g1_msm_strided(None, 4, 72, 0, 32, 64, 0, None, 4, None, 0, o) == 3
    assert lib.mi355zk_bn254_g1_msm_strided(p, 1 << 31, 72, 0, 32, 64, 0, None, 0, None, 0, o) == 3
    assert lib.mi355zk_bn254_g1_msm_strided(p, 8, 72, 0, 32, 64, 0, None, 0, None, 0, None) == 3


def test_rust_shim_takes_the_strided_path():
    src = open(RS).read()

    def body(fn):
        b = src[src.index("fn %s" % fn):]
        return b[:b.index("\n}\n")]

    for name in ("mi355zk_bn254_g1_msm_strided", "mi355zk_bn254_g2_msm_strided", "pin_shared(", "affine_layouts()"):
        assert name in body("try_multiexp"), name
    assert "mi355zk_bases_cache_pin_strided" in body("pin_shared")   # the pin, through the registry that holds the Arc
    assert "mi355zk_bases_cache_invalidate" in src and "strong_count" in src
    m = re.search(r"pub const MI355ZK_ABI_VERSION: c_int = (\d+);", src)
    h = re.search(r"#define MI355ZK_ABI_VERSION (\d+)", open(HDR).read())
    assert m and h and m.group(1) == h.group(1) == "7"
    patch = open(os.path.join(ROOT, "integration", "bellman_mi355zk.patch")).read()
    assert "fn shared_bases(&self)" in patch and "mi355zk_bn254_g1_msm_strided" in patch


def test_cpp_program_compiles_against_the_header():
    assert os.path.exists(build_cpp())
