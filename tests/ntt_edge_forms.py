"""Edge-value inputs of the Fr domain operations with their expected outputs in CLOSED FORM, on the STORED integers.

A domain operation is linear on the stored 256-bit words (the Montgomery factor is a common scalar), so for stored inputs a_i < r
    fft         X_k = sum_i a_i w^(ik)                 ifft         X_k = n^-1 sum_i a_i w^(-ik)
    coset_fft   X_k = sum_i a_i g^i w^(ik)             icoset_fft   X_k = g^-k * ifft(a)_k
with w = omega of the domain and g = 7 the coset generator, all as plain integers mod r.  With c = r - 1 (the largest canonical word
pattern) the patterns below put the largest values through every butterfly, make whole sub-transforms cancel to multiples of r (the tones:
n c at one output index and EXACTLY 0 at every other, so every reduction has to turn k r into 0 and subtractions meet equal operands) and
give the products operands at both ends of their range.  Every expected element costs at most one modular multiplication; no oracle.

cases(log_n, op) -> [(name, input (n, 4) uint64, expected (n, 4) uint64)].  For coset_fft the patterns are PRE-DIVIDED by g^i, so that the
pattern itself appears after distribute_powers, and the raw deltas are given too (closed form c g^j w^(jk)).
tests/test_ntt_closed_forms_host.py checks every form against the CPU oracle at 2^1 .. 2^10; tests/test_gpu_ntt_edges.py runs them on the device."""
import functools

import numpy as np

import bn254_model as M

R = M.R_ORDER
C = R - 1
G = M.FR_GENERATOR
GINV = pow(G, -1, R)
OPS = ["fft", "ifft", "coset_fft", "icoset_fft"]


def _rows(ints):
    """list of ints < 2^256 -> (n, 4) uint64"""
    return np.frombuffer(b"".join(v.to_bytes(32, "little") for v in ints), dtype=np.uint64).reshape(-1, 4).copy()


def _sparse(n, fill, entries):
    out = np.tile(np.array(M.to_limbs(fill), dtype=np.uint64), (n, 1))
    for i, v in entries.items():
        out[i] = M.to_limbs(v)
    return out


def _powers(base, n):
    out = [1] * n
    for i in range(1, n):
        out[i] = out[i - 1] * base % R
    return out


@functools.lru_cache(maxsize=None)
def _ginv_powers(n):
    return _powers(GINV, n)


class Vec:
    """a vector of n stored integers: dense (a list) or a fill value with a few other entries"""

    def __init__(self, n, fill=0, entries=None, dense=None):
        self.n, self.fill, self.entries, self.dense = n, fill, dict(entries or {}), dense

    def array(self):
        return _rows(self.dense) if self.dense is not None else _sparse(self.n, self.fill, self.entries)

    def times_powers(self, pw):
        """element i times pw[i]"""
        if self.dense is not None:
            return Vec(self.n, dense=[v * p % R for v, p in zip(self.dense, pw)])
        if self.fill == 0:
            return Vec(self.n, 0, {i: v * pw[i] % R for i, v in self.entries.items()})
        d = [self.fill * p % R for p in pw[:self.n]]
        for i, v in self.entries.items():
            d[i] = v * pw[i] % R
        return Vec(self.n, dense=d)


def _scaled_powers(first, base, n):
    """first * base^k, k < n: one multiplication per element"""
    out = [first % R] * n
    for k in range(1, n):
        out[k] = out[k - 1] * base % R
    return out


def _peaks(n, s, b, entries):
    """the vector that is v * s * b^k at the few indices k of `entries` and exactly 0 elsewhere"""
    return Vec(n, 0, {k: v * s % R * pow(b, k, R) % R for k, v in entries.items()})


def patterns(log_n, which="all"):
    """[(name, input Vec, form) ...]: form(e, s, b) is the closed form of  s * b^k * sum_i a_i w^(e i k)  (e = +1 / -1; s a scale; b = 1 or g^-1)."""
    n = 1 << log_n
    omega = M.domain_omega(log_n)
    half = n // 2
    out = []

    def add(name, vec, form):
        if which == "all" or name in which:
            out.append((name, vec, form))

    add("all zero", Vec(n), lambda e, s, b: Vec(n))
    add("all c", Vec(n, C), lambda e, s, b: _peaks(n, s, b, {0: n * C}))
    add("all one", Vec(n, 1), lambda e, s, b: _peaks(n, s, b, {0: n}))
    for j in sorted({0, 1, half, n - 1}):
        add("c at %d" % j, Vec(n, 0, {j: C}), lambda e, s, b, j=j: Vec(n, dense=_scaled_powers(C * s, pow(omega, e * j, R) * b % R, n)))   # c w^(jk)
    for odd in (0, 1):
        vec = Vec(n, dense=[C if i % 2 == 0 else odd for i in range(n)])
        add("c on even, %d on odd" % odd, vec, lambda e, s, b, odd=odd: _peaks(n, s, b, {half: (C - odd) * half, 0: (C + odd) * half}))
    winv = pow(omega, -1, R)
    for t in sorted({1 % n, half, n - 1}):
        vec = Vec(n, dense=_scaled_powers(C, pow(winv, t, R), n))                                  # a_i = c omega^(-t i): a single tone
        add("tone %d" % t, vec, lambda e, s, b, t=t: _peaks(n, s, b, {(e * t) % n: n * C}))        # n c at k = e t, exactly 0 elsewhere
    return out


def cases(log_n, op, which="all"):
    n = 1 << log_n
    omega = M.domain_omega(log_n)
    minv = pow(n, -1, R)
    out = []
    for name, vec, form in patterns(log_n, which):
        if op == "fft":
            out.append((name, vec, form(1, 1, 1)))
        elif op == "ifft":
            out.append((name, vec, form(-1, minv, 1)))
        elif op == "coset_fft":
            out.append((name + ", pre-divided by g^i", vec.times_powers(_ginv_powers(n)), form(1, 1, 1)))
            if name.startswith("c at "):
                j = int(name[5:])
                out.append((name + ", raw", vec, Vec(n, dense=_scaled_powers(C * pow(G, j, R), pow(omega, j, R), n))))   # c g^j w^(jk)
        else:
            out.append((name, vec, form(-1, minv, GINV)))
    return [(name, a.array(), x.array()) for name, a, x in out]
