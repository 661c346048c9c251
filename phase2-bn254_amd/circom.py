"""The producer side of the phase-2 ceremony, restated over the device library: the circom circuit reader and
`MPCParameters::new` -- the step that turns a constraint system and a `phase1radix2m{k}` file into the initial Groth16
parameters (the real "G1 + G2 mix" of BASELINE config 5).

Mirrored interfaces (same names, argument meaning and order of operations):
  phase2/src/circom_circuit.rs:46-56,332-360   CircuitJson / circuit_from_json: circuit.json of circom -> CircomCircuit
  phase2/src/circom_circuit.rs:319-331         witness_from_json
  phase2/src/circom_circuit.rs:135-185         Circuit::synthesize for CircomCircuit (variable 0 is the constant ONE)
  phase2/src/keypair_assembly.rs:15-25,70-105  KeypairAssembly: at / bt / ct, one (coefficient, constraint) list per variable
  phase2/src/parameters.rs:99-145              MPCParameters::new: the ONE input, synthesis, the `x * 0 = 0` input constraints,
                                               the domain size
  phase2/src/parameters.rs:225-400             eval (-> ceremony.eval_qap_polynomials: four sparse matrix x point-vector products
                                               on the device), UnconstrainedVariable, vk, the optional infinity filter, cs_hash

Host work here is what it is in the reference (JSON parsing, building the term lists); the group arithmetic -- one scalar
multiplication per (variable, constraint) term in G1 and, for the B polynomials, in G2 as well -- runs on the GPU.
"""
from __future__ import annotations

import json

import numpy as np

from . import ceremony
from .bellman import SynthesisError

_R_ORDER = ceremony._R_ORDER


def _fr_from_str(s: str) -> int:
    """PrimeField::from_str (ff_ce): decimal digits only, no sign, no leading zeros except "0" itself, value < r"""
    if not s or not s.isdigit() or (len(s) > 1 and s[0] == "0"):
        raise ValueError(f"not a field element: {s!r}")
    v = int(s)
    if v >= _R_ORDER:
        raise ValueError(f"not a field element: {s!r}")
    return v


class CircomCircuit:
    """circom_circuit.rs:99-111.  constraints: list of (A, B, C), each a list of (variable index, coefficient) with variable 0 the
    constant ONE, variables 1 .. num_inputs-1 the outputs and public inputs, the rest auxiliary."""

    def __init__(self, num_inputs: int, num_aux: int, num_constraints: int, constraints, witness=None):
        self.num_inputs, self.num_aux, self.num_constraints = num_inputs, num_aux, num_constraints
        self.constraints, self.witness = constraints, witness

    def get_public_inputs(self):
        return None if self.witness is None else list(self.witness[1:self.num_inputs])


def circuit_from_json(text) -> CircomCircuit:
    """circuit_from_json (circom_circuit.rs:340-360).  text: the JSON text (str / bytes) or an already parsed dict."""
    cj = text if isinstance(text, dict) else json.loads(text)
    num_inputs = int(cj["nPubInputs"]) + int(cj["nOutputs"]) + 1
    num_variables = int(cj["nVars"])
    num_aux = num_variables - num_inputs
    if num_aux < 0:
        raise ValueError("nVars < nPubInputs + nOutputs + 1")

    def index(k) -> int:
        # Rust's `parse::<usize>()` (circom_circuit.rs:346-350, unwrap): ASCII digits with an optional leading '+', nothing else
        # -- Python's int() would also take "-1", " 2" or "1_0", and a negative index would alias the LAST variable.  A variable
        # index past nVars panics in the reference when the constraint is synthesized; here it is rejected up front.
        digits = k[1:] if isinstance(k, str) and k.startswith("+") else k
        if not (isinstance(digits, str) and digits.isascii() and digits.isdigit()):
            raise ValueError(f"circuit.json: {k!r} is not a variable index")
        idx = int(digits)
        if idx >= num_variables:
            raise ValueError(f"circuit.json: variable index {idx} out of range (nVars = {num_variables})")
        return idx

    def convert(lc):   # a BTreeMap<String, String>: iterated in the order of the KEYS AS STRINGS
        return [(index(k), _fr_from_str(lc[k])) for k in sorted(lc.keys())]

    constraints = [(convert(c[0]), convert(c[1]), convert(c[2])) for c in cj["constraints"]]
    return CircomCircuit(num_inputs, num_aux, num_variables, constraints)


def circuit_from_json_file(path: str) -> CircomCircuit:
    with open(path, "rb") as f:
        return circuit_from_json(f.read())


def witness_from_json(text):
    return [_fr_from_str(x) for x in (text if isinstance(text, list) else json.loads(text))]


class KeypairAssembly:
    """keypair_assembly.rs:15-25: for every variable the (coefficient, constraint index) terms of its A, B and C polynomials, in
    the order the constraints were enforced.  Inputs first (index 0 = ONE), then the auxiliary variables."""

    def __init__(self):
        self.num_inputs = self.num_aux = self.num_constraints = 0
        self.at_inputs, self.bt_inputs, self.ct_inputs = [], [], []
        self.at_aux, self.bt_aux, self.ct_aux = [], [], []

    def alloc_input(self) -> int:
        self.num_inputs += 1
        for lst in (self.at_inputs, self.bt_inputs, self.ct_inputs):
            lst.append([])
        return self.num_inputs - 1

    def alloc(self) -> int:
        self.num_aux += 1
        for lst in (self.at_aux, self.bt_aux, self.ct_aux):
            lst.append([])
        return self.num_aux - 1

    def enforce(self, a, b, c):
        """a, b, c: lists of (is_input, index, coefficient)"""
        for lc, inputs, aux in ((a, self.at_inputs, self.at_aux), (b, self.bt_inputs, self.bt_aux), (c, self.ct_inputs, self.ct_aux)):
            for is_input, idx, coeff in lc:
                (inputs if is_input else aux)[idx].append((coeff, self.num_constraints))
        self.num_constraints += 1


def synthesize(circuit: CircomCircuit, cs: KeypairAssembly):
    """Circuit::synthesize (circom_circuit.rs:135-185) into a KeypairAssembly whose ONE input is already allocated."""
    for _ in range(1, circuit.num_inputs):
        cs.alloc_input()
    for _ in range(circuit.num_aux):
        cs.alloc()

    def lc(terms):
        # LinearCombination `+` appends; variable index < num_inputs is an input (0 = ONE), the rest auxiliary
        return [(idx < circuit.num_inputs, idx if idx < circuit.num_inputs else idx - circuit.num_inputs, coeff) for idx, coeff in terms]

    for a, b, c in circuit.constraints:
        cs.enforce(lc(a), lc(b), lc(c))


def _csr(rows, device):
    """per-variable term lists -> (row_ptr int32, col int32 = constraint / Lagrange index, coeff (nnz, 4) canonical limbs)"""
    import torch

    lens = np.fromiter((len(r) for r in rows), dtype=np.int64, count=len(rows))
    row_ptr = np.zeros(len(rows) + 1, dtype=np.int64)
    np.cumsum(lens, out=row_ptr[1:])
    nnz = int(row_ptr[-1])
    col = np.empty(nnz, dtype=np.int32)
    coeff = np.empty((nnz, 4), dtype=np.uint64)
    t = 0
    mask = (1 << 64) - 1
    for r in rows:
        for c, lag in r:
            col[t] = lag
            coeff[t, 0], coeff[t, 1], coeff[t, 2], coeff[t, 3] = c & mask, (c >> 64) & mask, (c >> 128) & mask, c >> 192
            t += 1
    return (torch.from_numpy(row_ptr.astype(np.int32)).to(device), torch.from_numpy(col).to(device),
            torch.from_numpy(coeff.view(np.int64)).to(device))


def domain_exponent(num_constraints: int) -> int:
    """parameters.rs:134-145: the power of two the evaluation domain needs"""
    m, exp = 1, 0
    while m < num_constraints:
        m *= 2
        exp += 1
        if exp > 28:
            raise SynthesisError(SynthesisError.POLYNOMIAL_DEGREE_TOO_LARGE)
    return exp


def assemble(circuit: CircomCircuit) -> KeypairAssembly:
    """parameters.rs:106-132: the ONE input, the circuit, and one `x * 0 = 0` constraint per input (full density of the IC query)"""
    cs = KeypairAssembly()
    cs.alloc_input()
    synthesize(circuit, cs)
    for i in range(cs.num_inputs):
        cs.enforce([(True, i, 1)], [], [])
    return cs


def mpc_parameters_new(circuit: CircomCircuit, should_filter_points_at_infinity: bool, radix):
    """MPCParameters::new (phase2/src/parameters.rs:99-400).  radix: what ceremony.read_phase1radix2m returned for
    phase1radix2m{domain_exponent(...)} (device records).  Returns the dict ceremony.write_mpc_parameters takes:
    {"params": {"vk", "h", "l", "a", "b_g1", "b_g2"}, "cs_hash": 64 bytes (device uint8), "contributions": []}."""
    import torch

    cs = assemble(circuit)
    m = 1 << domain_exponent(cs.num_constraints)
    if radix["coeffs_g1"].shape[0] != m:
        raise ValueError(f"the phase1radix2m file is for a domain of {radix['coeffs_g1'].shape[0]}, the circuit needs {m}")
    dev = radix["coeffs_g1"].device
    at = _csr(cs.at_inputs + cs.at_aux, dev)
    bt = _csr(cs.bt_inputs + cs.bt_aux, dev)
    ct = _csr(cs.ct_inputs + cs.ct_aux, dev)
    a_g1, b_g1, b_g2, ext = ceremony.eval_qap_polynomials(radix, at, bt, ct)
    ic, l = ext[:cs.num_inputs], ext[cs.num_inputs:]  # noqa: E741
    # "Don't allow any elements be unconstrained, so that the L query is always fully dense" (parameters.rs:340-346)
    if l.shape[0] and bool((l == 0).all(dim=1).any().item()):
        raise SynthesisError(SynthesisError.UNCONSTRAINED_VARIABLE)
    one1 = torch.from_numpy(ceremony.G1_ONE_RAW.view(np.int64).reshape(1, 8)).to(dev)
    one2 = torch.from_numpy(ceremony.G2_ONE_RAW.view(np.int64).reshape(1, 16)).to(dev)
    vk = {"alpha_g1": radix["alpha_g1"], "beta_g1": radix["beta_g1"], "beta_g2": radix["beta_g2"], "gamma_g2": one2, "delta_g1": one1,
          "delta_g2": one2, "ic": ic.contiguous()}
    if should_filter_points_at_infinity:
        keep = lambda pts: pts[~(pts == 0).all(dim=1)].contiguous()  # noqa: E731
        a_g1, b_g1, b_g2 = keep(a_g1), keep(b_g1), keep(b_g2)
    params = {"vk": vk, "h": radix["h"], "l": l.contiguous(), "a": a_g1, "b_g1": b_g1, "b_g2": b_g2}
    digest = ceremony.calculate_hash(ceremony.write_parameters(params))     # HashWriter over Parameters::write (parameters.rs:382-392)
    cs_hash = torch.frombuffer(bytearray(digest), dtype=torch.uint8).to(dev)
    return {"params": params, "cs_hash": cs_hash, "contributions": []}


# ---------------------------------------------------------------------------------------------------------------
# proving a circom circuit (circom_circuit.rs:187-191 `prove` = filter_params + create_random_proof; bellman's prepare_prover,
# groth16/prover.rs:49-200)
def prepare_prover(circuit: CircomCircuit, device):
    """prepare_prover (groth16/prover.rs:153-187): the ONE input, the circuit, one `x * 0 = 0` constraint per input, with the
    witness: per constraint the values of its A, B and C combinations, the assignments, and the three density maps (a variable
    counts as dense in a query as soon as it OCCURS in a combination, whatever its coefficient: prover.rs:49-88).  Returns the
    prover.ProvingAssignment (Montgomery Fr on the device, like Vec<Scalar<E>> / Vec<E::Fr>)."""
    import torch

    from . import prover as _prover
    from .bellman import DensityTracker

    if circuit.witness is None:
        raise SynthesisError("AssignmentMissing")
    w = circuit.witness
    if len(w) != circuit.num_inputs + circuit.num_aux:
        raise ValueError("the witness does not have one value per variable")
    num_inputs, num_aux = circuit.num_inputs, circuit.num_aux
    a_aux, b_in, b_aux = np.zeros(num_aux, dtype=bool), np.zeros(num_inputs, dtype=bool), np.zeros(num_aux, dtype=bool)
    a, b, c = [], [], []
    for ca, cb, cc in circuit.constraints:
        acc = 0
        for idx, coeff in ca:
            acc += coeff * w[idx]
            if idx >= num_inputs:
                a_aux[idx - num_inputs] = True
        a.append(acc % _R_ORDER)
        acc = 0
        for idx, coeff in cb:
            acc += coeff * w[idx]
            if idx >= num_inputs:
                b_aux[idx - num_inputs] = True
            else:
                b_in[idx] = True
        b.append(acc % _R_ORDER)
        c.append(sum(coeff * w[idx] for idx, coeff in cc) % _R_ORDER)
    for i in range(num_inputs):                      # x_i * 0 = 0
        a.append(w[i] % _R_ORDER)
        b.append(0)
        c.append(0)

    mont_r = (1 << 256) % _R_ORDER
    mask = (1 << 64) - 1

    def mont(vals):
        arr = np.empty((len(vals), 4), dtype=np.uint64)
        for i, v in enumerate(vals):
            v = v % _R_ORDER * mont_r % _R_ORDER
            arr[i, 0], arr[i, 1], arr[i, 2], arr[i, 3] = v & mask, (v >> 64) & mask, (v >> 128) & mask, v >> 192
        return torch.from_numpy(arr.view(np.int64)).to(device)

    return _prover.ProvingAssignment(mont(a), mont(b), mont(c), mont(w[:num_inputs]), mont(w[num_inputs:]), DensityTracker.from_bools(a_aux),
                                     DensityTracker.from_bools(b_in), DensityTracker.from_bools(b_aux))


# ---------------------------------------------------------------------------------------------------------------
# the same evaluation with the circuit COMPILED ONCE: what depends on the circuit and not on the witness (the term lists as one CSR
# matrix on the device, the density maps) is built by compile_circuit; every witness then costs one upload and two kernels
# (mi355zk_bn254_fr_from_repr_dev, mi355zk_bn254_fr_sparse_matvec_dev: csrc/r1cs.hip)
_MONT_R = (1 << 256) % _R_ORDER


def _limbs_array(vals) -> np.ndarray:
    """ints (< 2^256) -> (len, 4) u64 little-endian limbs"""
    buf = b"".join(int(v).to_bytes(32, "little") for v in vals)
    return np.frombuffer(buf, dtype=np.uint64).reshape(-1, 4).copy()


def _compile_host(circuit: CircomCircuit) -> dict:
    """The host half of compile_circuit (no device).  The rows prepare_prover evaluates -- one per constraint, then one `x_i * 0 = 0`
    row per input: n = len(constraints) + num_inputs -- padded with empty rows to m = 2^domain_exponent(n), for A, then B, then C: ONE
    CSR matrix of 3 m rows over the witness (col = variable index, inputs first), the coefficients deduplicated into a table of
    Montgomery forms.  Returns numpy arrays: row_ptr u32[3 m + 1], col u32[nnz], coeff_id u32[nnz], coeffs (n_coeffs, 4) u64, and the
    three DensityTrackers (a variable is dense as soon as it OCCURS; A tracks the aux variables only: prover.rs:49-88)."""
    from .bellman import DensityTracker

    num_inputs, num_aux = circuit.num_inputs, circuit.num_aux
    n_constraints = len(circuit.constraints)
    n = n_constraints + num_inputs
    exp = domain_exponent(n)
    m = 1 << exp
    table = {}
    lens = np.zeros(3 * m, dtype=np.int64)
    cols, ids, nnz_of = [], [], []
    for k in range(3):
        for i, constraint in enumerate(circuit.constraints):
            lc = constraint[k]
            lens[k * m + i] = len(lc)
            for idx, coeff in lc:
                cols.append(idx)
                ids.append(table.setdefault(coeff % _R_ORDER, len(table)))
        if k == 0:                                    # x_i * 0 = 0: the A combination is the input itself
            one = table.setdefault(1, len(table))
            lens[n_constraints:n] = 1
            cols.extend(range(num_inputs))
            ids.extend([one] * num_inputs)
        nnz_of.append(len(cols))
    col = np.asarray(cols, dtype=np.int64)
    if col.size and (int(col.min()) < 0 or int(col.max()) >= num_inputs + num_aux):
        raise ValueError("a constraint names a variable the circuit does not have")
    row_ptr = np.zeros(3 * m + 1, dtype=np.int64)
    np.cumsum(lens, out=row_ptr[1:])
    if int(row_ptr[-1]) >= 1 << 32 or len(table) >= 1 << 32:
        raise ValueError("the circuit has 2^32 terms or more")
    a_cols, b_cols = col[:nnz_of[0] - num_inputs], col[nnz_of[0]:nnz_of[1]]     # (the input rows of A hold inputs only)
    a_aux, b_in, b_aux = np.zeros(num_aux, dtype=bool), np.zeros(num_inputs, dtype=bool), np.zeros(num_aux, dtype=bool)
    a_aux[a_cols[a_cols >= num_inputs] - num_inputs] = True
    b_in[b_cols[b_cols < num_inputs]] = True
    b_aux[b_cols[b_cols >= num_inputs] - num_inputs] = True
    values = sorted(table, key=table.get)
    coeffs = _limbs_array(v * _MONT_R % _R_ORDER for v in values) if values else np.zeros((0, 4), dtype=np.uint64)
    return {"num_inputs": num_inputs, "num_aux": num_aux, "n": n, "exp": exp, "m": m,
            "row_ptr": row_ptr.astype(np.uint32), "col": col.astype(np.uint32), "coeff_id": np.asarray(ids, dtype=np.uint32), "coeffs": coeffs,
            "a_aux_density": DensityTracker.from_bools(a_aux), "b_input_density": DensityTracker.from_bools(b_in),
            "b_aux_density": DensityTracker.from_bools(b_aux)}


def _all_below_r(w: np.ndarray) -> bool:
    """every row of the (n, 4) u64 array, read as a little-endian integer, is < r"""
    mask = (1 << 64) - 1
    rl = [np.uint64((_R_ORDER >> (64 * i)) & mask) for i in range(4)]
    if not w.shape[0] or bool((w[:, 3] < rl[3]).all()):   # (the usual case: one pass over the top limbs)
        return True
    lt, eq = np.zeros(w.shape[0], dtype=bool), np.ones(w.shape[0], dtype=bool)
    for i in (3, 2, 1, 0):
        lt |= eq & (w[:, i] < rl[i])
        eq &= w[:, i] == rl[i]
    return bool(lt.all())


class CompiledCircuit:
    """A circuit's witness-independent half on a device (compile_circuit): the CSR matrix of _compile_host as device tensors (u32
    arrays as int32 views, the coefficient table as (n_coeffs, 4) int64) and the density maps."""

    def __init__(self, host: dict, device):
        import torch

        self.device = torch.device(device)
        self.num_inputs, self.num_aux, self.n, self.exp, self.m = (host[k] for k in ("num_inputs", "num_aux", "n", "exp", "m"))
        self.nnz, self.n_coeffs = int(host["col"].shape[0]), int(host["coeffs"].shape[0])
        up = lambda a, t: torch.from_numpy(np.ascontiguousarray(a).view(t)).to(self.device)  # noqa: E731
        self.row_ptr, self.col, self.coeff_id = up(host["row_ptr"], np.int32), up(host["col"], np.int32), up(host["coeff_id"], np.int32)
        self.coeffs = up(host["coeffs"], np.int64)
        self.a_aux_density, self.b_input_density, self.b_aux_density = host["a_aux_density"], host["b_input_density"], host["b_aux_density"]


def _cptr(t):
    import ctypes as C

    return C.c_void_p(t.data_ptr()) if t.numel() else None


def compile_circuit(circuit: CircomCircuit, device) -> CompiledCircuit:
    """Everything prepare_prover does that does not depend on the witness, once per circuit: the term lists of the A, B and C
    combinations as one CSR matrix on `device`, validated there once (mi355zk_bn254_fr_sparse_matvec_check_dev: the evaluating call
    does not report a bad index), and the three density maps.  The circuit's witness, if it has one, is not read."""
    import torch

    from . import lib as _lib
    from .bellman import DeviceError, _stream_ptr

    cc = CompiledCircuit(_compile_host(circuit), device)
    with torch.cuda.device(cc.device):
        rc = _lib.load().mi355zk_bn254_fr_sparse_matvec_check_dev(_cptr(cc.row_ptr), _cptr(cc.col), _cptr(cc.coeff_id), cc.n_coeffs,
                                                                  cc.num_inputs + cc.num_aux, 3 * cc.m, cc.nnz, _stream_ptr())
    if rc == _lib.ERR_BAD_ARGS:
        raise ValueError("mi355zk_bn254_fr_sparse_matvec_check_dev: the compiled matrix is not a valid CSR structure")
    if rc != 0:
        raise DeviceError(f"mi355zk fr_sparse_matvec_check failed rc={rc}")
    return cc


def _witness_limbs(n_vars: int, witness, who: str) -> np.ndarray:
    """One witness as prepare_prover_dev takes it -> (n_vars, 4) u64 canonical limbs; the refusals name `who`.  No device work."""
    if isinstance(witness, (list, tuple)):
        if len(witness) != n_vars:
            raise ValueError(f"{who} does not have one value per variable")
        return _limbs_array(v % _R_ORDER for v in witness) if n_vars else np.zeros((0, 4), dtype=np.uint64)
    w = np.ascontiguousarray(witness, dtype=np.uint64)
    if w.shape != (n_vars, 4):
        raise ValueError(f"{who} does not have one value of 4 x u64 per variable")
    if not _all_below_r(w):
        raise ValueError(f"{who} holds a value >= r: canonical values required")
    return w


def prepare_prover_dev(compiled: CompiledCircuit, witness):
    """prepare_prover on a compiled circuit.  witness: the list of ints witness_from_json returns, or an (n_vars, 4) u64 array of
    canonical values (a value >= r is a ValueError), inputs first.  One upload, the conversion to Montgomery form, ONE sparse product into a
    fresh (3 m, 4) tensor whose three m-row slices are a, b and c (their zero padding written by the empty rows: from_coeffs has
    nothing to append); the assignments are slices of the converted witness.  Same bytes and densities as prepare_prover."""
    import ctypes as C

    import torch

    from . import lib as _lib
    from . import prover as _prover
    from .bellman import DeviceError, _stream_ptr

    n_vars = compiled.num_inputs + compiled.num_aux
    w = _witness_limbs(n_vars, witness, "the witness")
    if not w.flags.writeable:
        w = w.copy()                                      # (torch.from_numpy wants a writable array; nothing is written)
    lib = _lib.load()
    m = compiled.m
    with torch.cuda.device(compiled.device):
        d_w = torch.from_numpy(w.view(np.int64)).to(compiled.device)
        out = torch.empty((3 * m, 4), dtype=torch.int64, device=compiled.device)
        rc = lib.mi355zk_bn254_fr_from_repr_dev(_cptr(d_w), _cptr(d_w), n_vars, _stream_ptr())
        if rc == 0:
            rc = lib.mi355zk_bn254_fr_sparse_matvec_dev(C.c_void_p(out.data_ptr()), _cptr(compiled.row_ptr), _cptr(compiled.col), _cptr(compiled.coeff_id),
                                                        _cptr(compiled.coeffs), compiled.n_coeffs, _cptr(d_w), n_vars, 3 * m, compiled.nnz, _stream_ptr())
    if rc != 0:
        raise DeviceError(f"mi355zk fr_sparse_matvec failed rc={rc}")
    return _prover.ProvingAssignment(out[:m], out[m:2 * m], out[2 * m:], d_w[:compiled.num_inputs], d_w[compiled.num_inputs:],
                                     compiled.a_aux_density, compiled.b_input_density, compiled.b_aux_density)


# ---------------------------------------------------------------------------------------------------------------
# a BATCH of witnesses of one circuit: one upload, one conversion, one product (mi355zk_bn254_fr_sparse_matvec_batch_dev: the matrix is
# the circuit's, as the base vectors are), and the check bellman's test constraint system has and its Groth16 path lacks -- is every
# constraint satisfied, and if not, which one (mi355zk_bn254_fr_r1cs_check_dev), before any multiexp is queued
_BATCH_PRODUCT = True   # profiles/r1cs_batch.md: the batch launch against the loop of single products


class UnsatisfiedConstraint(SynthesisError):
    """SynthesisError::Unsatisfiable (cs.rs:162) with what the device check found: `witness` (position in the batch), `index` (the
    lowest failing row of the matrix = circuit.constraints[index]), `count` (failing rows of that witness) and the row's three values
    a, b, c (canonical ints, a * b != c mod r)."""

    def __init__(self, witness: int, index: int, count: int, a: int, b: int, c: int):
        Exception.__init__(self, f"{SynthesisError.UNSATISFIABLE}: witness {witness} breaks constraint {index} (a * b != c); "
                                 f"{count} of its constraints fail")
        self.kind, self.index = SynthesisError.UNSATISFIABLE, index
        self.witness, self.count, self.a, self.b, self.c = witness, count, a, b, c


def prepare_provers_dev(compiled: CompiledCircuit, witnesses, check: bool = False):
    """prepare_prover_dev for B witnesses of one compiled circuit.  witnesses: a list of what prepare_prover_dev takes, or ONE
    (B, n_vars, 4) u64 array of canonical values; the refusals of prepare_prover_dev, before any device work, naming the witness.  ONE
    upload, ONE conversion over B * n_vars elements, ONE product into a fresh (B, 3 m, 4) tensor; assignment v's a, b, c and its
    input / aux assignments are views of these two tensors, the densities are the compiled circuit's, the bytes those of
    prepare_prover_dev per witness.  check=True: one first_unsatisfied over the batch; raises UnsatisfiedConstraint for the lowest
    failing witness at its first failing constraint.  Returns [ProvingAssignment]."""
    import ctypes as C

    import torch

    from . import lib as _lib
    from . import prover as _prover
    from .bellman import DeviceError, _stream_ptr

    n_vars = compiled.num_inputs + compiled.num_aux
    if isinstance(witnesses, np.ndarray):
        w = np.ascontiguousarray(witnesses, dtype=np.uint64)
        if w.ndim != 3 or w.shape[1:] != (n_vars, 4):
            raise ValueError("the witnesses are not a (B, n_vars, 4) array: one value of 4 x u64 per variable")
        for k in range(w.shape[0]):
            if not _all_below_r(w[k]):
                raise ValueError(f"witness {k} holds a value >= r: canonical values required")
    else:
        rows = [_witness_limbs(n_vars, wk, f"witness {k}") for k, wk in enumerate(witnesses)]
        w = np.stack(rows) if rows else np.zeros((0, n_vars, 4), dtype=np.uint64)
    n_batch = w.shape[0]
    if n_batch > _lib.R1CS_MAX_VECTORS:
        raise ValueError(f"more than {_lib.R1CS_MAX_VECTORS} witnesses in one batch")
    if n_batch == 0:
        return []
    if not w.flags.writeable:
        w = w.copy()                                      # (torch.from_numpy wants a writable array; nothing is written)
    lib = _lib.load()
    m = compiled.m
    matrix = (_cptr(compiled.row_ptr), _cptr(compiled.col), _cptr(compiled.coeff_id), _cptr(compiled.coeffs), compiled.n_coeffs)
    with torch.cuda.device(compiled.device):
        d_w = torch.from_numpy(w.view(np.int64)).to(compiled.device)
        out = torch.empty((n_batch, 3 * m, 4), dtype=torch.int64, device=compiled.device)
        rc = lib.mi355zk_bn254_fr_from_repr_dev(_cptr(d_w), _cptr(d_w), n_batch * n_vars, _stream_ptr())
        if rc == 0 and _BATCH_PRODUCT:
            rc = lib.mi355zk_bn254_fr_sparse_matvec_batch_dev(C.c_void_p(out.data_ptr()), 3 * m, *matrix, _cptr(d_w), n_vars, n_vars, n_batch,
                                                              3 * m, compiled.nnz, _stream_ptr())
        for v in range(0 if _BATCH_PRODUCT else n_batch):
            if rc == 0:
                rc = lib.mi355zk_bn254_fr_sparse_matvec_dev(C.c_void_p(out[v].data_ptr()), *matrix, _cptr(d_w[v]), n_vars, 3 * m, compiled.nnz, _stream_ptr())
    if rc != 0:
        raise DeviceError(f"mi355zk fr_sparse_matvec_batch failed rc={rc}")
    provers = [_prover.ProvingAssignment(out[v, :m], out[v, m:2 * m], out[v, 2 * m:], d_w[v, :compiled.num_inputs], d_w[v, compiled.num_inputs:],
                                         compiled.a_aux_density, compiled.b_input_density, compiled.b_aux_density) for v in range(n_batch)]
    if check:
        _raise_if_unsatisfied(provers)
    return provers


def _r1cs_check(tensors, n_rows: int, stride: int, n_vectors: int):
    """one mi355zk_bn254_fr_r1cs_check_dev over n_vectors vectors that start at the three tensors and lie `stride` elements apart"""
    import ctypes as C

    import torch

    from . import lib as _lib
    from .bellman import DeviceError, _stream_ptr

    first = (C.c_longlong * n_vectors)()
    count = (C.c_uint32 * n_vectors)()
    with torch.cuda.device(tensors[0].device):
        rc = _lib.load().mi355zk_bn254_fr_r1cs_check_dev(_cptr(tensors[0]), _cptr(tensors[1]), _cptr(tensors[2]), n_rows, stride, n_vectors,
                                                         first, count, _stream_ptr())
    if rc != 0:
        raise DeviceError(f"mi355zk fr_r1cs_check failed rc={rc}")
    return [(None if first[v] < 0 else int(first[v]), int(count[v])) for v in range(n_vectors)]


def first_unsatisfied(assignments):
    """Is a[i] * b[i] == c[i] in every row: [(index of the lowest failing row or None, number of failing rows)], one pair per
    ProvingAssignment (one assignment or a list of them, of any origin: prepare_prover, prepare_prover_dev, prepare_provers_dev).
    ONE device call when the assignments are equally spaced slices of one allocation (what prepare_provers_dev returns), one call
    each otherwise.  The call waits for the device."""
    from . import prover as _prover

    provers = [assignments] if isinstance(assignments, _prover.ProvingAssignment) else list(assignments)
    if not provers:
        return []
    abc = []
    for p in provers:
        t = [x if x.is_contiguous() else x.contiguous() for x in (p.a, p.b, p.c)]
        if not all(x.is_cuda and x.dim() == 2 and x.shape == t[0].shape and x.shape[1] == 4 and x.element_size() == 8 for x in t):
            raise ValueError("first_unsatisfied: a, b and c are not three (n, 4) 64-bit device tensors of one length")
        abc.append(t)
    n_rows = abc[0][0].shape[0]
    stride_bytes = abc[1][0].data_ptr() - abc[0][0].data_ptr() if len(abc) > 1 else 32 * n_rows
    one_call = stride_bytes >= 32 * n_rows and stride_bytes % 32 == 0 and all(
        t[k].shape[0] == n_rows and t[k].device == abc[0][0].device
        and t[k].untyped_storage().data_ptr() == abc[0][k].untyped_storage().data_ptr()
        and t[k].data_ptr() - abc[0][k].data_ptr() == v * stride_bytes for v, t in enumerate(abc) for k in range(3))
    if one_call:
        return _r1cs_check(abc[0], n_rows, stride_bytes // 32, len(abc))
    return [_r1cs_check(t, t[0].shape[0], t[0].shape[0], 1)[0] for t in abc]


def _raise_if_unsatisfied(provers):
    """UnsatisfiedConstraint for the lowest witness of `provers` with a failing row, the row's three values copied back (96 bytes)"""
    import torch

    for v, (index, count) in enumerate(first_unsatisfied(provers)):
        if index is not None:
            p = provers[v]
            row = torch.stack([p.a[index], p.b[index], p.c[index]]).cpu().numpy().view(np.uint64).reshape(3, 4)
            r_inv = pow(_MONT_R, -1, _R_ORDER)
            a, b, c = (int.from_bytes(row[k].tobytes(), "little") * r_inv % _R_ORDER for k in range(3))
            raise UnsatisfiedConstraint(v, index, count, a, b, c)


def filter_params(params):
    """filter_params (circom_circuit.rs:271-277): vk.ic, h, a, b_g1 and b_g2 without their points at infinity (the A / B queries
    are what the density maps index; l is left as it is, as in the reference)."""
    keep = lambda pts: pts[~(pts == 0).all(dim=1)].contiguous()  # noqa: E731
    vk = dict(params["vk"], ic=keep(params["vk"]["ic"]))
    return dict(params, vk=vk, h=keep(params["h"]), a=keep(params["a"]), b_g1=keep(params["b_g1"]), b_g2=keep(params["b_g2"]))


def prove(pool, circuit: CircomCircuit, params, r: int, s: int, compiled: CompiledCircuit = None, check: bool = False):
    """prove (circom_circuit.rs:187-191) with the blinding scalars given (create_random_proof draws them from the RNG):
    returns the proof (a, b, c) as raw affine records.  params: the "params" dict of mpc_parameters_new / read_mpc_parameters.
    compiled: compile_circuit(circuit, device) -- the witness is then evaluated on the device (prepare_prover_dev); same proof.
    check: first_unsatisfied on the assignment; an unsatisfied witness raises UnsatisfiedConstraint before any multiexp is queued."""
    from . import prover as _prover

    p = filter_params(params)
    host = lambda t: t.cpu().numpy().view(np.uint64).reshape(-1)  # noqa: E731
    vk = {k: host(p["vk"][k]) for k in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2")}
    if compiled is None:
        assignment = prepare_prover(circuit, p["h"].device)
    else:
        if circuit.witness is None:
            raise SynthesisError("AssignmentMissing")
        if (compiled.num_inputs, compiled.num_aux, compiled.n) != (circuit.num_inputs, circuit.num_aux, len(circuit.constraints) + circuit.num_inputs):
            raise ValueError("`compiled` was not compiled from this circuit (variable or constraint counts differ)")
        assignment = prepare_prover_dev(compiled, circuit.witness)
    if check:
        _raise_if_unsatisfied([assignment])
    return _prover.create_proof(pool, _prover.Parameters(vk, p["h"], p["l"], p["a"], p["b_g1"], p["b_g2"]), assignment, r, s)


def prove_many(pool, circuit: CircomCircuit, params, witnesses, rs, ss, compiled: CompiledCircuit = None, check: bool = False):
    """prove for many witnesses of one circuit: prepare_provers_dev over ONE CompiledCircuit (compiled here when the caller brings
    none) -- one upload, one conversion, one product for the batch -- then prover.create_proofs -- every multiexp of the batch in one
    pipeline.  witnesses: what prepare_provers_dev takes, one per proof; rs, ss: the blinding scalars, one pair per proof.  check: the
    first unsatisfied witness raises UnsatisfiedConstraint before any multiexp is queued.  Returns [(a, b, c)]: what prove returns for
    each witness."""
    from . import prover as _prover

    p = filter_params(params)
    host = lambda t: t.cpu().numpy().view(np.uint64).reshape(-1)  # noqa: E731
    vk = {k: host(p["vk"][k]) for k in ("alpha_g1", "beta_g1", "delta_g1", "beta_g2", "delta_g2")}
    if compiled is None:
        compiled = compile_circuit(circuit, p["h"].device)
    if (compiled.num_inputs, compiled.num_aux, compiled.n) != (circuit.num_inputs, circuit.num_aux, len(circuit.constraints) + circuit.num_inputs):
        raise ValueError("`compiled` was not compiled from this circuit (variable or constraint counts differ)")
    assignments = prepare_provers_dev(compiled, witnesses, check=check)
    return _prover.create_proofs(pool, _prover.Parameters(vk, p["h"], p["l"], p["a"], p["b_g1"], p["b_g2"]), assignments, rs, ss)
