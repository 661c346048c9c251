"""The H-polynomial entry points, host side (no GPU): mi355zk_bn254_fr_h_combine_dev, mi355zk_bn254_fr_h_poly_dev and
mi355zk_bn254_fr_h_poly are declared, exported and bound; every argument rule of include/mi355zk.h returns 3 (bad arguments) before any
device work -- this process has no device, so a rule checked too late would come back as a device failure (< 0), not 3; and the Rust shim's
try_h_poly goes through the host-buffer entry.  (The chain itself runs in tests/test_gpu_h_poly.py.)"""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RS = os.path.join(ROOT, "integration", "mi355zk.rs")
HDR = os.path.join(ROOT, "include", "mi355zk.h")
NEW = ["mi355zk_bn254_fr_h_combine_dev", "mi355zk_bn254_fr_h_poly_dev", "mi355zk_bn254_fr_h_poly"]
BAD_ARGS = 3


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
    assert re.search(r"#define\s+MI355ZK_H_INTO_REPR\s+1u", text) and zk.lib.H_INTO_REPR == 1
    assert lib.mi355zk_abi_version() == zk.lib.ABI_VERSION == 7   # symbols were added, no prototype changed


def _p(x):
    return C.c_void_p(x)


# fake, distinct, non-null "device" addresses: a refused call must not touch them
DA, DB, DC = 0x10000, 0x20000, 0x30000


def test_h_combine_dev_bad_arguments(lib):
    f = lib.mi355zk_bn254_fr_h_combine_dev
    assert f(_p(None), _p(DB), _p(DC), 4, 2, None) == BAD_ARGS
    assert f(_p(DA), _p(None), _p(DC), 4, 2, None) == BAD_ARGS
    assert f(_p(DA), _p(DB), _p(None), 4, 2, None) == BAD_ARGS
    assert f(_p(DA), _p(DB), _p(DC), 4, 29, None) == BAD_ARGS
    assert f(_p(None), _p(None), _p(None), 0, 29, None) == BAD_ARGS   # log_n is checked whatever n is
    assert f(_p(None), _p(None), _p(None), 0, 3, None) == 0           # nothing to do: no pointer is needed, no device either


def test_h_poly_dev_bad_arguments(lib):
    f = lib.mi355zk_bn254_fr_h_poly_dev
    assert f(_p(None), _p(DB), _p(DC), 4, 0, None) == BAD_ARGS
    assert f(_p(DA), _p(None), _p(DC), 4, 0, None) == BAD_ARGS
    assert f(_p(DA), _p(DB), _p(None), 4, 0, None) == BAD_ARGS
    assert f(_p(DA), _p(DA), _p(DC), 4, 0, None) == BAD_ARGS    # a repeated pointer: a == b
    assert f(_p(DA), _p(DB), _p(DA), 4, 0, None) == BAD_ARGS    # a == c
    assert f(_p(DA), _p(DB), _p(DB), 4, 0, None) == BAD_ARGS    # b == c
    assert f(_p(DA), _p(DB), _p(DC), 29, 0, None) == BAD_ARGS   # PolynomialDegreeTooLarge
    assert f(_p(DA), _p(DB), _p(DC), 4, 2, None) == BAD_ARGS    # unknown flag bits
    assert f(_p(DA), _p(DB), _p(DC), 4, 1 | 4, None) == BAD_ARGS


def test_h_poly_host_bad_arguments(lib):
    f = lib.mi355zk_bn254_fr_h_poly
    n = 16
    a, b, c = (np.full((n, 4), k, dtype=np.uint64) for k in (1, 2, 3))
    h = np.full((n, 4), 9, dtype=np.uint64)
    p = lambda x: x.ctypes.data_as(C.c_void_p)   # noqa: E731
    assert f(_p(None), p(a), p(b), p(c), n, 4, 0) == BAD_ARGS
    assert f(p(h), _p(None), p(b), p(c), n, 4, 0) == BAD_ARGS
    assert f(p(h), p(a), _p(None), p(c), n, 4, 0) == BAD_ARGS
    assert f(p(h), p(a), p(b), _p(None), n, 4, 0) == BAD_ARGS
    assert f(p(h), p(a), p(b), p(c), 0, 4, 0) == BAD_ARGS        # len == 0
    assert f(p(h), p(a), p(b), p(c), n + 1, 4, 0) == BAD_ARGS    # len > 2^log_n
    assert f(p(h), p(a), p(b), p(c), 2, 0, 0) == BAD_ARGS        # len > 2^0
    assert f(p(h), p(a), p(b), p(c), n, 29, 0) == BAD_ARGS       # log_n > 28
    assert f(p(h), p(a), p(b), p(c), n, 4, 2) == BAD_ARGS        # unknown flag bits
    assert f(p(a), p(a), p(b), p(c), n, 4, 0) == BAD_ARGS        # h == a
    assert f(p(b), p(a), p(b), p(c), n, 4, 0) == BAD_ARGS        # h == b
    assert f(p(c), p(a), p(b), p(c), n, 4, 0) == BAD_ARGS        # h == c
    # a refused call wrote nothing anywhere
    assert (a == 1).all() and (b == 2).all() and (c == 3).all() and (h == 9).all()


def test_python_bindings_refuse_bad_arguments():
    import phase2_bn254_amd as zk

    a = np.ones((5, 4), dtype=np.uint64)
    with pytest.raises(ValueError):
        zk.bellman.h_poly_host(a, a[:4], a, 3)            # three lengths
    with pytest.raises(ValueError):
        zk.bellman.h_poly_host(a, a.copy(), a.copy(), 2)  # len > 2^log_n: the library's rc 3
    with pytest.raises(zk.SynthesisError):
        zk.bellman.h_poly_host(a, a.copy(), a.copy(), 29)
    assert zk.h_poly_host is zk.bellman.h_poly_host and hasattr(zk.EvaluationDomain, "h_poly")


def test_rust_shim_try_h_poly_calls_the_host_entry():
    src = open(RS).read()
    m = re.search(r"pub fn try_h_poly<.*?\n}\n", src, flags=re.S)
    assert m, "integration/mi355zk.rs has no try_h_poly"
    body = m.group(0)
    assert src.index("// ---- END GENERATED ----") < m.start()            # hand-written, below the generated block
    assert re.search(r"\bmi355zk_bn254_fr_h_poly\s*\(", body)
    assert "-> Option<" in body and re.search(r"if rc != 0 \{\s*return None;", body)   # ANY non-zero rc: the caller's CPU path
    assert "MI355ZK_H_INTO_REPR" in body and re.search(r"pub const MI355ZK_H_INTO_REPR: u32 = 1;", src)
    assert re.search(r"pub fn mi355zk_bn254_fr_h_poly\(h: \*mut u64, a: \*const u64, b: \*const u64, c: \*const u64, len: usize, log_n: u32, flags: u32\) -> c_int;", src)
