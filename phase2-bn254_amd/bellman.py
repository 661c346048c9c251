"""Host-side mirror of the reference's interface for the accelerated path (thin; all compute is in
libmi355zk.so through the C ABI).  The C++ twin of this file is host/bellman.hpp.

Reference interface mirrored (same names, argument meaning, error behaviour):
  bellman/src/multiexp.rs:330-340   multiexp(pool, bases, density_map, exponents) -> Future<Projective>
  bellman/src/source.rs:36-140      (Arc<Vec<G>>, usize) source builder, FullDensity, DensityTracker
  bellman/src/domain.rs:30-203      EvaluationDomain::{from_coeffs, fft, ifft, coset_fft, icoset_fft, ...}
  bellman/src/multicore.rs:17-72    Worker
  bellman/src/cs.rs:156-173         SynthesisError variants raised on this path

Data may live on the host (numpy uint64 arrays -> host-buffer entry points) or already in HBM
(torch CUDA tensors of dtype int64/uint64 -> `_dev` entry points on torch's current stream).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import lib as _lib

FR_S = 28  # Fr::S, pairing/src/bn256/fr.rs:31-34


class SynthesisError(Exception):
    """bellman/src/cs.rs:156-173 (the variants this path can raise)."""

    UNEXPECTED_IDENTITY = "UnexpectedIdentity"          # source.rs:50-52
    IO_UNEXPECTED_EOF = "IoError(UnexpectedEof)"        # source.rs:46-48,62-64
    POLYNOMIAL_DEGREE_TOO_LARGE = "PolynomialDegreeTooLarge"  # domain.rs:66-79
    UNCONSTRAINED_VARIABLE = "UnconstrainedVariable"    # phase2/src/parameters.rs:340-346 (MPCParameters::new)
    MALFORMED_VERIFYING_KEY = "MalformedVerifyingKey"   # groth16/verifier.rs:40-42 (verify_proof)
    UNSATISFIABLE = "Unsatisfiable"                     # cs.rs:162 (circom.UnsatisfiedConstraint: the witness check on the device)

    def __init__(self, kind: str, index: int = -1):
        super().__init__(kind if index < 0 else f"{kind} at exponent {index}")
        self.kind = kind
        self.index = index


class DeviceError(RuntimeError):
    """HIP failure inside libmi355zk (no reference counterpart; there is no CPU fallback)."""


class Worker:
    """bellman/src/multicore.rs:17-35.  The reference's Worker is a CPU thread pool; here it names the GPU(s) the calling process
    drives.  Worker(3): one GPU (one process per GPU, shard.py).  Worker(devices=[0, 1, .., 7]): the single-process multi-GPU mode
    of mi355zk_init -- host-buffer multiexps of >= 2^20 exponents are cut into one point range per device and joined on the host,
    shorter ones go to the devices in turn (include/mi355zk.h).  The last Worker constructed defines the library's device set."""

    def __init__(self, device: int | None = None, devices=None):
        if devices is not None:
            devices = [int(d) for d in devices]
            assert devices and device is None
            ids = (C.c_int * len(devices))(*devices)
            self.device, self.devices, n = devices[0], devices, len(devices)
        else:
            ids = (C.c_int * 1)(device) if device is not None else None
            self.device, self.devices, n = device, [device] if device is not None else [], 1 if device is not None else 0
        rc = _lib.load().mi355zk_init(ids, n)
        if rc != 0:
            raise DeviceError(f"mi355zk_init failed (rc={rc})")

    def log_num_cpus(self) -> int:  # multicore.rs:37-39; serial/parallel FFT split is moot on the GPU
        return 0


class FullDensity:
    """source.rs:80-99"""

    def get_query_size(self):
        return None

    def words(self):
        return None, 0


class DensityTracker:
    """source.rs:101-140 (BitVec-backed in the reference; here a numpy uint32 word array with the
    ABI's bit order: bit i = word i/32, bit i%32)."""

    def __init__(self):
        self._bits = np.zeros(64, dtype=np.uint8)   # one byte per element, grown geometrically (add_element is called per variable)
        self._n = 0
        self.total_density = 0
        self._packed = None                         # words() of the current contents (a proof asks for the same map 2-3 times)

    def add_element(self):
        if self._n == self._bits.size:
            self._bits = np.concatenate([self._bits, np.zeros(self._bits.size, dtype=np.uint8)])
        self._bits[self._n] = 0
        self._n += 1
        self._packed = None

    def inc(self, idx: int):
        if idx >= self._n:
            raise IndexError(idx)
        if not self._bits[idx]:
            self._bits[idx] = 1
            self.total_density += 1
            self._packed = None

    def get_total_density(self) -> int:
        return self.total_density

    def get_query_size(self):
        return self._n

    @classmethod
    def from_bools(cls, bools) -> "DensityTracker":
        d = cls()
        d._bits = np.ascontiguousarray(np.asarray(bools, dtype=bool), dtype=np.uint8).reshape(-1)
        d._n = d._bits.size
        if d._n == 0:
            d._bits = np.zeros(64, dtype=np.uint8)
        d.total_density = int(d._bits[:d._n].sum())
        return d

    def words(self):
        if self._packed is None:
            n = self._n
            w = np.zeros((n + 31) // 32 or 1, dtype=np.uint32)
            if n:
                pad = np.zeros(w.size * 32, dtype=np.uint8)
                pad[:n] = self._bits[:n]
                w[:] = np.packbits(pad.reshape(-1, 32), axis=1, bitorder="little").view(np.uint32).reshape(-1)
            self._packed = (w, n)
        return self._packed


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _stream_ptr():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


class _Ready:
    """A completed future (futures 0.1 `future::result`): multiexp() is synchronous here, which is
    what singlecore::Worker::compute already is in the reference (singlecore.rs:33-47)."""

    def __init__(self, value=None, error: Exception | None = None):
        self._value, self._error = value, error

    def wait(self):
        if self._error is not None:
            raise self._error
        return self._value


class StridedBases:
    """A host base vector in the CALLER's record layout: `data` is (n, stride) u8, record i = data[i]; x / y are the 32 (G1) or 64 (G2,
    c0 || c1) Montgomery bytes at x_off / y_off; inf_off is the offset of a flag byte that makes the record the identity when non-zero
    (None: no flag).  multiexp / pin_bases / unpin_bases take it where a packed (n, 8) / (n, 16) array goes; the library repacks the
    records on the device (mi355zk_bn254_g{1,2}_msm_strided, mi355zk_bases_cache_pin_strided)."""

    def __init__(self, data, group: int, x_off: int, y_off: int, inf_off=None):
        assert not _is_torch(data) and data.dtype == np.uint8 and data.ndim == 2 and data.flags["C_CONTIGUOUS"]
        assert group in (1, 2)
        self.data, self.group = data, group
        self.stride, self.x_off, self.y_off = int(data.shape[1]), int(x_off), int(y_off)
        self.inf_off = None if inf_off is None else int(inf_off)

    def __len__(self):
        return int(self.data.shape[0])

    @property
    def layout(self):
        return (self.stride, self.x_off, self.y_off, _lib.NO_FLAG if self.inf_off is None else self.inf_off)

    def ptr(self):
        return self.data.ctypes.data_as(C.c_void_p)

    @classmethod
    def _affine_rust(cls, group: int, x, y, infinity, pad: int):
        # pairing's `G1Affine { x: Fq, y: Fq, infinity: bool }` / G2Affine (ec.rs:14-18): the coordinates, the flag byte, padding to 8 B
        limbs = 4 * group
        x = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1, limbs)
        y = np.ascontiguousarray(y, dtype=np.uint64).reshape(-1, limbs)
        n, csz = x.shape[0], 32 * group
        stride = 2 * csz + 8
        data = np.full((n, stride), pad, dtype=np.uint8)
        data[:, :csz] = x.view(np.uint8).reshape(n, csz)
        data[:, csz:2 * csz] = y.view(np.uint8).reshape(n, csz)
        data[:, 2 * csz] = np.asarray(infinity, dtype=bool).reshape(n) if infinity is not None else 0
        return cls(data, group, 0, csz, 2 * csz)

    @classmethod
    def g1_affine_rust(cls, x, y, infinity=None, pad: int = 0) -> "StridedBases":
        """72-byte records x || y || infinity || 7 padding bytes (value `pad`) from (n, 4) u64 x / y limbs and a boolean mask."""
        return cls._affine_rust(1, x, y, infinity, pad)

    @classmethod
    def g2_affine_rust(cls, x, y, infinity=None, pad: int = 0) -> "StridedBases":
        """136-byte records x.c0 || x.c1 || y.c0 || y.c1 || infinity || 7 padding bytes from (n, 8) u64 x / y limbs and a mask."""
        return cls._affine_rust(2, x, y, infinity, pad)


def pin_bases(arr, tables: bool = False) -> None:
    """mi355zk_bases_cache_pin: declare the HOST base vector `arr` ((n, 8) / (n, 16) u64, C-contiguous) immutable until
    unpin_bases(arr) -- the `Arc<Vec<G>>` of a Parameters object (groth16/mod.rs:216-238).  Host-buffer multiexps over it then
    keep their uploaded copy on the device.  Without the promise every call uploads its bases again.  A StridedBases pins under its
    layout (mi355zk_bases_cache_pin_strided; the device copy is packed)."""
    if isinstance(arr, StridedBases):
        rc = _lib.load().mi355zk_bases_cache_pin_strided(arr.ptr(), len(arr), *arr.layout, arr.group, _lib.PIN_TABLES if tables else 0)
        if rc != 0:
            raise ValueError("mi355zk_bases_cache_pin_strided: bad arguments")
        return
    assert not _is_torch(arr) and arr.flags["C_CONTIGUOUS"] and arr.dtype == np.uint64
    fn = _lib.load().mi355zk_bases_cache_pin_tables if tables else _lib.load().mi355zk_bases_cache_pin  # tables: + the window table (table mode)
    rc = fn(arr.ctypes.data_as(C.c_void_p), arr.shape[0], {8: 1, 16: 2}[arr.shape[1]])
    if rc != 0:
        raise ValueError("mi355zk_bases_cache_pin: bad arguments")


def unpin_bases(arr=None) -> None:
    """mi355zk_bases_cache_invalidate: the promise ends (before rewriting or freeing the vector); None: every vector."""
    if isinstance(arr, StridedBases):
        arr = arr.data   # (every layout pinned at the pointer goes)
    _lib.load().mi355zk_bases_cache_invalidate(arr.ctypes.data_as(C.c_void_p) if arr is not None else None)


class MsmTable:
    """The window table of a device-resident base vector (mi355zk_bn254_g{1,2}_msm_table_build_dev): pass `(table, offset)` to
    multiexp() where `(bases, offset)` would go -- same result and errors, evaluated in table mode (one bucket set for all windows).
    For vectors that stay put between calls: the `Arc<Vec<G>>` of groth16::Parameters (groth16/mod.rs:216-238)."""

    def __init__(self, bases):
        import torch

        assert _is_torch(bases) and bases.is_cuda and bases.is_contiguous() and bases.shape[1] in (8, 16)
        lib = _lib.load()
        self.n_bases, self.limbs = int(bases.shape[0]), int(bases.shape[1])
        self.group = {8: 1, 16: 2}[self.limbs]
        c, w = C.c_uint32(), C.c_uint32()
        if lib.mi355zk_msm_table_geometry(self.n_bases, self.group, C.byref(c), C.byref(w)) != 0:
            raise ValueError("mi355zk_msm_table_geometry: bad arguments")
        self.window_bits, self.n_windows = int(c.value), int(w.value)
        self.table = torch.empty((self.n_windows * self.n_bases, self.limbs), dtype=torch.int64, device=bases.device)
        fn = lib.mi355zk_bn254_g1_msm_table_build_dev if self.group == 1 else lib.mi355zk_bn254_g2_msm_table_build_dev
        with torch.cuda.device(bases.device):
            rc = fn(C.c_void_p(bases.data_ptr()), self.n_bases, C.c_void_p(self.table.data_ptr()), self.table.numel() * 8, _stream_ptr())
        if rc != 0:
            raise DeviceError(f"mi355zk msm_table_build rc={rc}")


class FixedBaseTable:
    """The window table of ONE base point for fixed-base scalar multiplication (mi355zk_bn254_g{1,2}_fixed_base_build_dev): what
    `Wnaf::base(g, n)` is to groth16/generator.rs:178-510.  `base` is a raw affine record ((8,) / (16,) u64, host), a non-infinite point of
    the order-r group; anything else raises ValueError.  mul(scalars) returns the affine records of scalars[i] * base as an (n, 8) / (n, 16)
    int64 device tensor (all-zero = infinity); it is asynchronous on the current stream."""

    def __init__(self, base, device=None):
        import torch

        base = np.ascontiguousarray(np.asarray(base, dtype=np.uint64).reshape(-1))
        assert base.size in (8, 16)
        lib = _lib.load()
        self.limbs = int(base.size)
        self.group = {8: 1, 16: 2}[self.limbs]
        nbytes = int(lib.mi355zk_fixed_base_table_bytes(self.group))
        self.device = torch.device("cuda") if device is None else torch.device(device)
        if self.device.index is None:
            self.device = torch.device("cuda", torch.cuda.current_device())
        self.table = torch.empty(nbytes // 8, dtype=torch.int64, device=self.device)   # (the entry format is the library's own)
        fn = lib.mi355zk_bn254_g1_fixed_base_build_dev if self.group == 1 else lib.mi355zk_bn254_g2_fixed_base_build_dev
        with torch.cuda.device(self.device):
            rc = fn(C.c_void_p(self.table.data_ptr()), nbytes, base.ctypes.data_as(C.c_void_p), _stream_ptr())
        if rc == _lib.ERR_BAD_ARGS:
            raise ValueError("fixed_base_build: the base is not a non-infinite point of the order-r group")
        if rc != 0:
            raise DeviceError(f"mi355zk fixed_base_build rc={rc}")

    def mul(self, scalars, montgomery: bool = False):
        """scalars: (n, 4) int64 device tensor of canonical FrRepr, or of Montgomery Fr with montgomery=True"""
        import torch

        assert _is_torch(scalars) and scalars.is_cuda and scalars.is_contiguous() and scalars.dtype == torch.int64 and scalars.device == self.device
        n = scalars.numel() // 4
        out = torch.empty((n, self.limbs), dtype=torch.int64, device=self.device)
        fn = _lib.load().mi355zk_bn254_g1_fixed_base_mul_dev if self.group == 1 else _lib.load().mi355zk_bn254_g2_fixed_base_mul_dev
        with torch.cuda.device(self.device):
            rc = fn(C.c_void_p(out.data_ptr()), C.c_void_p(self.table.data_ptr()), C.c_void_p(scalars.data_ptr()), n,
                    _lib.FIXED_SCALARS_MONTGOMERY if montgomery else 0, _stream_ptr())
        if rc != 0:
            raise DeviceError(f"mi355zk fixed_base_mul rc={rc}")
        return out


def multiexp(pool: Worker, bases, density_map, exponents, window_group=None, scalars_montgomery: bool = False) -> _Ready:
    """bellman/src/multiexp.rs:330.  (window_group = (groups, index), device-resident data only: the partial sum over one
    of `groups` equal groups of scalar windows -- multi-GPU sharding by windows, shard.py; None = the whole multiexp.
    scalars_montgomery, device-resident data only: `exponents` are Montgomery-form Fr elements, i.e. the prover's vectors BEFORE
    scalars_into_representations / field_elements_into_representations (prover.rs:89-129); the conversion is fused into the call.)  `bases` = (array, offset) like `(Arc<Vec<G>>, usize)`:
    array of shape (n_bases, 8) u64 for G1Affine raw records or (n_bases, 16) for G2Affine;
    or a StridedBases (host records in the caller's layout, e.g. pairing's 72-byte G1Affine);
    `exponents` = (n, 4) u64 canonical FrRepr; `density_map` = FullDensity() or a DensityTracker.
    Returns a ready future whose wait() yields the Jacobian X||Y||Z limbs (12 / 24 u64)."""
    arr, offset = bases
    qs = density_map.get_query_size()
    n_exp = int(exponents.shape[0])
    if qs is not None:
        assert qs == n_exp  # multiexp.rs:347-352
    words, dbits = density_map.words()
    lib = _lib.load()
    if isinstance(arr, MsmTable):
        import torch

        if window_group is not None and tuple(window_group) != (1, 0):
            raise ValueError("table mode evaluates all windows in one bucket set: no window groups")
        assert exponents.is_cuda and exponents.is_contiguous()
        out = np.zeros(12 * arr.group, dtype=np.uint64)
        fn = lib.mi355zk_bn254_g1_msm_table_dev if arr.group == 1 else lib.mi355zk_bn254_g2_msm_table_dev
        with torch.cuda.device(arr.table.device):
            rc = fn(C.c_void_p(arr.table.data_ptr()), arr.n_bases, offset, C.c_void_p(exponents.data_ptr()), n_exp,
                    words.ctypes.data_as(C.c_void_p) if words is not None else None, dbits,
                    _lib.MSM_SCALARS_MONTGOMERY if scalars_montgomery else 0, _stream_ptr(), out.ctypes.data_as(C.c_void_p))
    elif isinstance(arr, StridedBases):
        if (window_group is not None and tuple(window_group) != (1, 0)) or scalars_montgomery:
            raise ValueError("window groups / Montgomery scalars need device-resident inputs")
        exponents = np.ascontiguousarray(exponents, dtype=np.uint64)
        out = np.zeros(12 * arr.group, dtype=np.uint64)
        fn = lib.mi355zk_bn254_g1_msm_strided if arr.group == 1 else lib.mi355zk_bn254_g2_msm_strided
        rc = fn(arr.ptr(), len(arr), *arr.layout, offset, exponents.ctypes.data_as(C.c_void_p), n_exp,
                words.ctypes.data_as(C.c_void_p) if words is not None else None, dbits, out.ctypes.data_as(C.c_void_p))
    elif _is_torch(arr):
        import torch

        assert arr.is_cuda and exponents.is_cuda and arr.is_contiguous() and exponents.is_contiguous()
        limbs = arr.shape[1]
        group = {8: 1, 16: 2}[limbs]
        out = np.zeros(12 * group, dtype=np.uint64)
        wg, wi = window_group if window_group is not None else (1, 0)
        fn = lib.mi355zk_bn254_g1_msm_ex_dev if group == 1 else lib.mi355zk_bn254_g2_msm_ex_dev
        with torch.cuda.device(arr.device):
            rc = fn(C.c_void_p(arr.data_ptr()), arr.shape[0], offset, C.c_void_p(exponents.data_ptr()), n_exp,
                    words.ctypes.data_as(C.c_void_p) if words is not None else None, dbits,
                    _lib.MSM_SCALARS_MONTGOMERY if scalars_montgomery else 0, int(wg), int(wi), _stream_ptr(), out.ctypes.data_as(C.c_void_p))
    else:
        if (window_group is not None and tuple(window_group) != (1, 0)) or scalars_montgomery:
            raise ValueError("window groups / Montgomery scalars need device-resident inputs")
        arr = np.ascontiguousarray(arr, dtype=np.uint64)
        exponents = np.ascontiguousarray(exponents, dtype=np.uint64)
        limbs = arr.shape[1] if arr.ndim == 2 else 8
        group = {8: 1, 16: 2}[limbs]
        out = np.zeros(12 * group, dtype=np.uint64)
        fn = lib.mi355zk_bn254_g1_msm if group == 1 else lib.mi355zk_bn254_g2_msm
        rc = fn(arr.ctypes.data_as(C.c_void_p), arr.shape[0], offset, exponents.ctypes.data_as(C.c_void_p), n_exp,
                words.ctypes.data_as(C.c_void_p) if words is not None else None, dbits, out.ctypes.data_as(C.c_void_p))
    if rc == _lib.OK:
        return _Ready(out)
    idx = int(lib.mi355zk_last_error_index())
    if rc == _lib.ERR_UNEXPECTED_IDENTITY:
        return _Ready(error=SynthesisError(SynthesisError.UNEXPECTED_IDENTITY, idx))
    if rc == _lib.ERR_UNEXPECTED_EOF:
        return _Ready(error=SynthesisError(SynthesisError.IO_UNEXPECTED_EOF, idx))
    if rc == _lib.ERR_BAD_ARGS:
        return _Ready(error=ValueError("mi355zk: bad arguments"))
    return _Ready(error=DeviceError(f"mi355zk device failure rc={rc}"))


def multiexp_many(pool: Worker, bases, density_map, exponents, scalars_montgomery: bool = False) -> list:
    """B multiexps over ONE base vector and ONE density map in one call (mi355zk_bn254_g{1,2}_msm_batch_dev): the shape of "many proofs
    over one Parameters".  `exponents`: a contiguous (B, n, 4) int64 device tensor, vector v = exponents[v]; `bases` = (tensor, offset)
    or (MsmTable, offset) -- a table's window 0 is the vector itself (msm_table_build_dev), so the batch runs over table[:n_bases].
    Returns B ready futures; future v carries what multiexp(pool, bases, density_map, exponents[v], ...) would: the Jacobian limbs, or
    the same SynthesisError / ValueError / DeviceError."""
    import torch

    arr, offset = bases
    assert _is_torch(exponents) and exponents.is_cuda and exponents.is_contiguous() and exponents.dim() == 3 and exponents.shape[2] == 4
    n_vec, n_exp = int(exponents.shape[0]), int(exponents.shape[1])
    qs = density_map.get_query_size()
    if qs is not None:
        assert qs == n_exp  # multiexp.rs:347-352
    words, dbits = density_map.words()
    if isinstance(arr, MsmTable):
        dev_bases, n_bases, limbs = arr.table, arr.n_bases, arr.limbs
    else:
        assert _is_torch(arr) and arr.is_cuda and arr.is_contiguous()
        dev_bases, n_bases, limbs = arr, int(arr.shape[0]), int(arr.shape[1])
    group = {8: 1, 16: 2}[limbs]
    if n_vec == 0:
        return []
    lib = _lib.load()
    out = np.zeros((n_vec, 12 * group), dtype=np.uint64)
    rcs = np.zeros(n_vec, dtype=np.int32)
    idxs = np.full(n_vec, -1, dtype=np.int64)
    fn = lib.mi355zk_bn254_g1_msm_batch_dev if group == 1 else lib.mi355zk_bn254_g2_msm_batch_dev
    with torch.cuda.device(dev_bases.device):
        rc = fn(C.c_void_p(dev_bases.data_ptr()), n_bases, offset, C.c_void_p(exponents.data_ptr()), n_exp, n_exp, n_vec,
                words.ctypes.data_as(C.c_void_p) if words is not None else None, dbits,
                _lib.MSM_SCALARS_MONTGOMERY if scalars_montgomery else 0, _stream_ptr(), out.ctypes.data_as(C.c_void_p),
                rcs.ctypes.data_as(C.c_void_p), idxs.ctypes.data_as(C.c_void_p))
    if rc != _lib.OK:   # the call as a whole: every vector carries it
        rcs[:] = rc

    def ready(v):
        code, idx = int(rcs[v]), int(idxs[v])
        if code == _lib.OK:
            return _Ready(out[v].copy())
        if code == _lib.ERR_UNEXPECTED_IDENTITY:
            return _Ready(error=SynthesisError(SynthesisError.UNEXPECTED_IDENTITY, idx))
        if code == _lib.ERR_UNEXPECTED_EOF:
            return _Ready(error=SynthesisError(SynthesisError.IO_UNEXPECTED_EOF, idx))
        if code == _lib.ERR_BAD_ARGS:
            return _Ready(error=ValueError("mi355zk: bad arguments"))
        return _Ready(error=DeviceError(f"mi355zk device failure rc={code}"))

    return [ready(v) for v in range(n_vec)]


class EvaluationDomain:
    """bellman/src/domain.rs:30-203 for G = Scalar<Bn256>: coefficients are (m, 4) u64 Montgomery Fr
    limbs, either a numpy array or a torch CUDA tensor (int64 view)."""

    def __init__(self, coeffs, exp: int):
        self.coeffs = coeffs
        self.exp = exp

    @classmethod
    def from_coeffs(cls, coeffs) -> "EvaluationDomain":
        n = int(coeffs.shape[0])
        if n > (1 << FR_S) - 1:  # domain.rs:66-68
            raise SynthesisError(SynthesisError.POLYNOMIAL_DEGREE_TOO_LARGE)
        m, exp = 1, 0
        while m < n:  # domain.rs:70-79
            m *= 2
            exp += 1
            if exp > FR_S:
                raise SynthesisError(SynthesisError.POLYNOMIAL_DEGREE_TOO_LARGE)
        if m != n:  # coeffs.resize(m, G::group_zero()), domain.rs:89
            if _is_torch(coeffs):
                import torch

                pad = torch.zeros((m - n, 4), dtype=coeffs.dtype, device=coeffs.device)
                coeffs = torch.cat([coeffs, pad]).contiguous()
            else:
                coeffs = np.concatenate([np.asarray(coeffs, dtype=np.uint64), np.zeros((m - n, 4), dtype=np.uint64)])
        elif not _is_torch(coeffs):
            coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64).copy()
        else:
            # `from_coeffs` takes the Vec by value (domain.rs:52): the domain owns its coefficients and the transforms work in
            # place, so the caller's tensor is copied -- a ProvingAssignment can then be proved twice
            coeffs = coeffs.contiguous().clone()
        return cls(coeffs, exp)

    def as_ref(self):
        return self.coeffs

    def into_coeffs(self):
        return self.coeffs

    def _op(self, op: int):
        lib = _lib.load()
        if _is_torch(self.coeffs):
            import torch

            assert self.coeffs.is_cuda and self.coeffs.is_contiguous()
            with torch.cuda.device(self.coeffs.device):
                rc = lib.mi355zk_bn254_fr_domain_op_dev(C.c_void_p(self.coeffs.data_ptr()), self.exp, op, _stream_ptr())
        else:
            rc = lib.mi355zk_bn254_fr_domain_op(self.coeffs.ctypes.data_as(C.c_void_p), self.exp, op)
        if rc != 0:
            raise DeviceError(f"mi355zk NTT failed rc={rc}")

    @staticmethod
    def _op_many(domains, op: int):
        """The same operation on several device-resident domains of one size (prover.rs:217-241: a, b, c): one launch per pass over all of
        them (mi355zk_bn254_fr_domain_op_batch_dev) -- the results are those of the separate calls, byte for byte."""
        domains = list(domains)
        if not domains:
            return
        d0 = domains[0]
        if len(domains) == 1 or not all(_is_torch(d.coeffs) and d.coeffs.is_cuda and d.exp == d0.exp and d.coeffs.device == d0.coeffs.device for d in domains):
            for d in domains:
                d._op(op)
            return
        import torch

        ptrs = (C.c_void_p * len(domains))(*[d.coeffs.data_ptr() for d in domains])
        assert all(d.coeffs.is_contiguous() for d in domains)
        with torch.cuda.device(d0.coeffs.device):
            rc = _lib.load().mi355zk_bn254_fr_domain_op_batch_dev(ptrs, len(domains), d0.exp, op, _stream_ptr())
        if rc != 0:
            raise DeviceError(f"mi355zk batched NTT failed rc={rc}")

    @staticmethod
    def fft_many(worker: Worker, domains):
        EvaluationDomain._op_many(domains, _lib.OP_FFT)

    @staticmethod
    def ifft_many(worker: Worker, domains):
        EvaluationDomain._op_many(domains, _lib.OP_IFFT)

    @staticmethod
    def coset_fft_many(worker: Worker, domains):
        EvaluationDomain._op_many(domains, _lib.OP_COSET_FFT)

    @staticmethod
    def icoset_fft_many(worker: Worker, domains):
        EvaluationDomain._op_many(domains, _lib.OP_ICOSET_FFT)

    def fft(self, worker: Worker):  # domain.rs:154
        self._op(_lib.OP_FFT)

    def ifft(self, worker: Worker):  # domain.rs:159
        self._op(_lib.OP_IFFT)

    def coset_fft(self, worker: Worker):  # domain.rs:191
        self._op(_lib.OP_COSET_FFT)

    def icoset_fft(self, worker: Worker):  # domain.rs:197
        self._op(_lib.OP_ICOSET_FFT)

    # ---- the elementwise steps of the prover's H pipeline (prover.rs:217-241), device-resident coefficients only
    def _dev_coeffs(self):
        if not _is_torch(self.coeffs):
            raise ValueError("device-resident coefficients (a torch CUDA tensor) required")
        return C.c_void_p(self.coeffs.data_ptr())

    def _on_device(self):
        """context manager: the coefficients' GPU is current (kernels and `_stream_ptr()` then refer to ITS stream, not to the
        stream of whatever device the caller last selected)"""
        import torch

        self._dev_coeffs()
        return torch.cuda.device(self.coeffs.device)

    def z(self, tau):
        """domain.rs:207-212: tau^m - 1 (tau, result: 4 u64 Montgomery limbs)."""
        tau = np.ascontiguousarray(tau, dtype=np.uint64)
        out = np.zeros(4, dtype=np.uint64)
        rc = _lib.load().mi355zk_bn254_fr_domain_z(self.exp, tau.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p))
        if rc != 0:
            raise DeviceError(f"mi355zk domain_z failed rc={rc}")
        return out

    def divide_by_z_on_coset(self, worker: Worker):  # domain.rs:217-234
        with self._on_device():
            rc = _lib.load().mi355zk_bn254_fr_divide_by_z_on_coset_dev(self._dev_coeffs(), self.exp, _stream_ptr())
        if rc != 0:
            raise DeviceError(f"mi355zk divide_by_z_on_coset failed rc={rc}")

    def mul_assign(self, worker: Worker, other: "EvaluationDomain"):  # domain.rs:236-249
        assert self.coeffs.shape[0] == other.coeffs.shape[0]
        assert other.coeffs.device == self.coeffs.device
        with self._on_device():
            rc = _lib.load().mi355zk_bn254_fr_mul_assign_dev(self._dev_coeffs(), other._dev_coeffs(), self.coeffs.shape[0], _stream_ptr())
        if rc != 0:
            raise DeviceError(f"mi355zk mul_assign failed rc={rc}")

    def sub_assign(self, worker: Worker, other: "EvaluationDomain"):  # domain.rs:251-260
        assert self.coeffs.shape[0] == other.coeffs.shape[0]
        assert other.coeffs.device == self.coeffs.device
        with self._on_device():
            rc = _lib.load().mi355zk_bn254_fr_sub_assign_dev(self._dev_coeffs(), other._dev_coeffs(), self.coeffs.shape[0], _stream_ptr())
        if rc != 0:
            raise DeviceError(f"mi355zk sub_assign failed rc={rc}")

    @staticmethod
    def h_poly(a: "EvaluationDomain", b: "EvaluationDomain", c: "EvaluationDomain", worker: Worker, into_repr: bool = False) -> "EvaluationDomain":
        """The prover's H evaluation (prover.rs:216-248) on three device-resident domains of one size, in ONE library call
        (mi355zk_bn254_fr_h_poly_dev): ifft and coset_fft of a, b, c, a = (a * b - c) / z in one elementwise pass, icoset_fft and, with
        into_repr, the conversion to canonical FrRepr.  Returns `a`, whose coefficients hold the result -- the caller drops the last one
        (prover.rs:243-246); b and c are scratch afterwards.  Byte for byte what the ten separate calls leave."""
        ta, tb, tc = a.coeffs, b.coeffs, c.coeffs
        if not all(_is_torch(t) and t.is_cuda and t.is_contiguous() for t in (ta, tb, tc)):
            raise ValueError("device-resident coefficients (contiguous torch CUDA tensors) required")
        assert a.exp == b.exp == c.exp and ta.shape[0] == tb.shape[0] == tc.shape[0] == 1 << a.exp
        assert ta.device == tb.device == tc.device
        with a._on_device():
            rc = _lib.load().mi355zk_bn254_fr_h_poly_dev(C.c_void_p(ta.data_ptr()), C.c_void_p(tb.data_ptr()), C.c_void_p(tc.data_ptr()), a.exp,
                                                         _lib.H_INTO_REPR if into_repr else 0, _stream_ptr())
        if rc == _lib.ERR_BAD_ARGS:
            raise ValueError("mi355zk_bn254_fr_h_poly_dev: bad arguments")
        if rc != 0:
            raise DeviceError(f"mi355zk h_poly failed rc={rc}")
        return a


def h_poly_host(a, b, c, log_n: int, into_repr: bool = False):
    """The same chain on HOST arrays (mi355zk_bn254_fr_h_poly): a, b, c are (len, 4) u64 Montgomery Fr with len <= 2^log_n, zero-padded
    by the library as `from_coeffs` does; returns the (2^log_n - 1, 4) coefficients of h (canonical FrRepr with into_repr).  One upload
    of the three arrays and one download, instead of seven round trips through mi355zk_bn254_fr_domain_op.  The inputs are not written."""
    arrs = [np.ascontiguousarray(x, dtype=np.uint64) for x in (a, b, c)]
    if not all(x.ndim == 2 and x.shape[1] == 4 and x.shape[0] == arrs[0].shape[0] for x in arrs):
        raise ValueError("a, b, c: three (len, 4) u64 arrays of one length")
    if not 0 <= log_n <= FR_S:
        raise SynthesisError(SynthesisError.POLYNOMIAL_DEGREE_TOO_LARGE)
    h = np.empty(((1 << log_n) - 1, 4), dtype=np.uint64)
    hp = h.ctypes.data_as(C.c_void_p) if h.size else np.empty((1, 4), dtype=np.uint64).ctypes.data_as(C.c_void_p)
    rc = _lib.load().mi355zk_bn254_fr_h_poly(hp, *[x.ctypes.data_as(C.c_void_p) for x in arrs], arrs[0].shape[0], log_n,
                                             _lib.H_INTO_REPR if into_repr else 0)
    if rc == _lib.ERR_BAD_ARGS:
        raise ValueError("mi355zk_bn254_fr_h_poly: bad arguments")
    if rc != 0:
        raise DeviceError(f"mi355zk h_poly failed rc={rc}")
    return h


def best_fft(a, worker: Worker, omega, log_n: int):
    """bellman/src/domain.rs:263: in-place transform of `a` (numpy (2^log_n, 4) u64) with root `omega`."""
    rc = _lib.load().mi355zk_bn254_fr_ntt(a.ctypes.data_as(C.c_void_p), log_n,
                                          np.ascontiguousarray(omega, dtype=np.uint64).ctypes.data_as(C.c_void_p))
    if rc != 0:
        raise DeviceError(f"mi355zk NTT failed rc={rc}")
