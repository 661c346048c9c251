"""Running products and running sums of device-resident Fr rows (csrc/fr_scan.hip), and what the reference builds from them.

  prefix_products, prefix_sums     out[i] = a[0] o .. o a[i] (inclusive) or a[0] o .. o a[i-1] (exclusive), per row
  ratio_products, ratio_sums       the same over term[i] = num[i] / den[i]: ONE field inversion per call, no array of terms
  mul_add                          a[i] += c b[i]   (mul_add_polynomials, bellman/src/sonic/util.rs:855-873; b None: a[i] += c)
  grand_product_polynomials        GrandProductArgument::new (sonic/unhelped/grand_product_argument.rs:94-172): for every pair (a, b) the
                                   polynomials a || 0 || b and prefix(a) || 1 || prefix(b) of length 2 n + 1, and v = (prod a)^-1
  permutation_product              Z[0] = 1, Z[i+1] = Z[i] num[i] / den[i] with num = prod_j (values_j + beta positions_j + gamma) and den the
                                   same over the permuted positions (permutation_argument.rs:286-420 feeds the argument above with these
                                   terms): the accumulator of a PLONK-style permutation check, and its total

Conventions as in kzg.py: arrays are int64 device tensors of Montgomery Fr, (n, 4) for one row or (rows, n, 4); scalars (beta, gamma, c) are
Python ints mod r.  A 3-d tensor may be a VIEW with a row stride (t[:, lo:hi]): rows are addressed by stride, nothing is copied.  A zero is an
ordinary element of a product -- everything after it in its row is zero, as in the serial chain; only a zero DENOMINATOR is an error.
The results are arrays that kzg.commit_many takes as they are."""
from __future__ import annotations

import ctypes as C

from . import kzg
from . import lib as _lib
from .bellman import _stream_ptr
from .kzg import _check, _mont_rows


def _layout(t, what: str):
    """(rows, n, row stride in elements) of an (n, 4) or (rows, n, 4) int64 device tensor whose rows are dense"""
    ok = getattr(t, "is_cuda", False) and t.dim() in (2, 3) and t.shape[-1] == 4 and t.element_size() == 8
    if ok and t.numel():
        ok = t.stride(-1) == 1 and (t.shape[-2] == 1 or t.stride(-2) == 4) and \
            (t.dim() == 2 or t.shape[0] == 1 or (t.stride(0) % 4 == 0 and t.stride(0) >= 4 * t.shape[1]))
    if not ok:
        raise ValueError(f"{what}: an (n, 4) or (rows, n, 4) int64 device tensor of Montgomery Fr with dense rows")
    rows, n = (1, int(t.shape[0])) if t.dim() == 2 else (int(t.shape[0]), int(t.shape[1]))
    if rows > _lib.SCAN_MAX_ROWS:
        raise ValueError(f"{what}: at most {_lib.SCAN_MAX_ROWS} rows per call")
    stride = int(t.stride(0)) // 4 if t.dim() == 3 and rows > 1 and t.numel() else n
    return rows, n, stride


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None


def _out_like(a, out, what: str):
    import torch

    if out is None:
        return torch.empty(tuple(a.shape), dtype=torch.int64, device=a.device)
    if not (getattr(out, "is_cuda", False) and tuple(out.shape) == tuple(a.shape) and out.dtype == a.dtype and out.device == a.device):
        raise ValueError(f"{what}: out has the input's shape, dtype and device")
    return out


def _totals(a, rows: int):
    import torch

    return torch.empty((rows, 4) if a.dim() == 3 else (4,), dtype=torch.int64, device=a.device)


def _scan(a, flags: int, out, total: bool, what: str):
    import torch

    rows, n, a_stride = _layout(a, what)
    out = _out_like(a, out, what)
    _, _, out_stride = _layout(out, what)
    tot = _totals(a, rows) if total else None
    with torch.cuda.device(a.device):
        _check(_lib.load().mi355zk_bn254_fr_scan_dev(_ptr(out), out_stride, _ptr(a), a_stride, n, rows, flags, _ptr(tot) if rows else None,
                                                     _stream_ptr()), what)
    return (out, tot) if total else out


def prefix_products(a, exclusive=False, out=None, total=False):
    """Running products per row: out[i] = a[0] .. a[i], or with `exclusive` out[0] = 1, out[i] = a[0] .. a[i-1].  out: None (a new tensor), `a`
    itself (in place) or a tensor of a's shape that does not overlap it.  total: also return every row's product, (rows, 4) or (4,)."""
    return _scan(a, _lib.SCAN_EXCLUSIVE if exclusive else 0, out, total, "prefix_products")


def prefix_sums(a, exclusive=False, out=None, total=False):
    """Running sums per row; arguments as prefix_products (the identity is zero)."""
    return _scan(a, _lib.SCAN_SUM | (_lib.SCAN_EXCLUSIVE if exclusive else 0), out, total, "prefix_sums")


def _ratio(num, den, flags: int, out, total: bool, allow_zero: bool, what: str):
    import torch

    rows, n, den_stride = _layout(den, what)
    num_stride = 0
    if num is not None:
        if tuple(num.shape) != tuple(den.shape) or getattr(num, "device", None) != den.device:
            raise ValueError(f"{what}: num has den's shape and device")
        _, _, num_stride = _layout(num, what)
    out = _out_like(den, out, what)
    _, _, out_stride = _layout(out, what)
    tot = _totals(den, rows) if total else None
    with torch.cuda.device(den.device):
        zeros = torch.empty(1, dtype=torch.int32, device=den.device)
        _check(_lib.load().mi355zk_bn254_fr_ratio_scan_dev(_ptr(out), out_stride, _ptr(num), num_stride, _ptr(den), den_stride, n, rows, flags,
                                                           _ptr(tot) if rows else None, C.c_void_p(zeros.data_ptr()), _stream_ptr()), what)
        n_zero = int(zeros.item()) & 0xFFFFFFFF
    if n_zero and not allow_zero:
        raise ZeroDivisionError(f"{what}: {n_zero} zero denominator{'s' if n_zero != 1 else ''}")
    res = (out,) + ((tot,) if total else ()) + ((n_zero,) if allow_zero else ())
    return res if len(res) > 1 else out


def ratio_products(num, den, exclusive=True, out=None, total=False, allow_zero=False):
    """The running product of num[i] / den[i] per row (num None: of 1 / den[i]); by default exclusive, Z[0] = 1 and Z[i+1] = Z[i] num[i] / den[i].
    out may be den (the denominators are inverted where the result goes), not num.  A zero denominator raises ZeroDivisionError naming their
    number; with allow_zero its term counts as zero and the number is returned last.  Returns out[, totals][, zeros]; waits for the device."""
    return _ratio(num, den, _lib.SCAN_EXCLUSIVE if exclusive else 0, out, total, allow_zero, "ratio_products")


def ratio_sums(num, den, exclusive=True, out=None, total=False, allow_zero=False):
    """The running sum of num[i] / den[i] per row (the log-derivative lookup sum); arguments as ratio_products."""
    return _ratio(num, den, _lib.SCAN_SUM | (_lib.SCAN_EXCLUSIVE if exclusive else 0), out, total, allow_zero, "ratio_sums")


def mul_add(a, b, c):
    """a[i] += c b[i] in place on `a`, a contiguous (..., 4) device tensor; b None: a[i] += c.  c is an int mod r.  Returns a."""
    import torch

    if not (getattr(a, "is_cuda", False) and a.dim() >= 1 and a.shape[-1] == 4 and a.element_size() == 8 and a.is_contiguous()):
        raise ValueError("mul_add: a contiguous (..., 4) int64 device tensor of Montgomery Fr")
    if b is not None and not (getattr(b, "is_cuda", False) and tuple(b.shape) == tuple(a.shape) and b.dtype == a.dtype and b.device == a.device
                              and b.is_contiguous()):
        raise ValueError("mul_add: b has a's shape, dtype and device")
    cm = _mont_rows([c])
    with torch.cuda.device(a.device):
        _check(_lib.load().mi355zk_bn254_fr_mul_add_dev(_ptr(a), _ptr(b), cm.ctypes.data_as(C.c_void_p), a.numel() // 4, _stream_ptr()), "fr_mul_add")
    return a


def _mul_assign(a, b):
    import torch

    with torch.cuda.device(a.device):
        _check(_lib.load().mi355zk_bn254_fr_mul_assign_dev(_ptr(a), _ptr(b), a.numel() // 4, _stream_ptr()), "fr_mul_assign")


def grand_product_polynomials(pairs):
    """GrandProductArgument::new for P pairs (a, b) of (n, 4) tensors of one length n >= 1: (a_polys, c_polys, v) with
    a_polys[p] = a || 0 || b and c_polys[p] = prefix(a) || 1 || prefix(b), both (P, 2 n + 1, 4), and v[p] = (prod a)^-1, (P, 4).  Two scans of P
    rows each write straight into c_polys, one batch inversion gives v.  The reference asserts c[n-1] == c[2n]; here a pair whose two products
    differ raises ValueError naming the first such pair."""
    import torch

    pairs = list(pairs)
    if not pairs:
        raise ValueError("grand_product_polynomials: at least one pair")
    n, dev = int(pairs[0][0].shape[0]), pairs[0][0].device
    for a, b in pairs:
        for t in (a, b):
            if not (getattr(t, "is_cuda", False) and t.dim() == 2 and tuple(t.shape) == (n, 4) and t.element_size() == 8 and t.device == dev) or n == 0:
                raise ValueError("grand_product_polynomials: every a and b is an (n, 4) int64 device tensor of one length n >= 1")
    p = len(pairs)
    with torch.cuda.device(dev):
        a_polys = torch.zeros((p, 2 * n + 1, 4), dtype=torch.int64, device=dev)
        a_polys[:, :n] = torch.stack([a for a, _ in pairs])
        a_polys[:, n + 1:] = torch.stack([b for _, b in pairs])
        c_polys = torch.empty((p, 2 * n + 1, 4), dtype=torch.int64, device=dev)
        c_polys[:, n] = torch.from_numpy(_mont_rows([1])[0].view("int64")).to(dev)
        _, prod_a = prefix_products(a_polys[:, :n], out=c_polys[:, :n], total=True)
        _, prod_b = prefix_products(a_polys[:, n + 1:], out=c_polys[:, n + 1:], total=True)
        differ = (prod_a != prod_b).any(dim=1).nonzero()
        if differ.numel():
            raise ValueError(f"grand_product_polynomials: the products of pair {int(differ[0])} differ (b is not a permutation of a)")
        v = kzg.batch_inverse(prod_a)
    return a_polys, c_polys, v


def _permutation_terms(values, positions, beta: int, gamma: int):
    """prod_j (values_j + beta positions_j + gamma) as an (n, 4) tensor: two mul_add per column and a mul_assign_dev per column after the first,
    3 k - 1 small launches (the 2 k + 2 of three columns)"""
    acc = None
    for j in range(int(values.shape[0])):
        term = values[j].clone()
        mul_add(term, positions[j], beta)
        mul_add(term, None, gamma)
        if acc is None:
            acc = term
        else:
            _mul_assign(acc, term)
    return acc


def permutation_product(values, positions, permuted, beta, gamma):
    """The permutation accumulator over k columns of n rows: values, positions, permuted are (k, n, 4) tensors.
    num[i] = prod_j (values[j, i] + beta positions[j, i] + gamma), den[i] the same with permuted; Z[0] = 1, Z[i+1] = Z[i] num[i] / den[i].
    Returns (Z: (n, 4), total: (4,) = Z[n]).  The total is Montgomery one exactly when the multisets {(value, position)} and {(value, permuted)}
    agree; for a false statement it is one only with probability about n k / r over beta, gamma.  A zero denominator raises ZeroDivisionError."""
    for t in (values, positions, permuted):
        if not (getattr(t, "is_cuda", False) and t.dim() == 3 and t.shape[2] == 4 and t.element_size() == 8 and tuple(t.shape) == tuple(values.shape)
                and t.shape[0] >= 1 and t.is_contiguous()):
            raise ValueError("permutation_product: values, positions and permuted are contiguous (k, n, 4) int64 device tensors of one shape, k >= 1")
    num = _permutation_terms(values, positions, int(beta), int(gamma))
    den = _permutation_terms(values, permuted, int(beta), int(gamma))
    z, total = ratio_products(num, den, exclusive=True, out=den, total=True)
    return z, total
