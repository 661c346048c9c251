"""Satisfied circuits and witnesses for the witness-batch tests (tests/test_witness_check_host.py, tests/test_gpu_witness_batch.py), the
ways to break chosen rows of them, and the big-int verdict of the satisfaction check."""
import numpy as np

import r1cs_cases as K

R_ORDER = K.R_ORDER


class Satisfied:
    """circuit: a zk.circom.CircomCircuit whose witness satisfies every constraint.  Its variables are num_inputs inputs (0 = ONE),
    n_shared - num_inputs shared auxiliary variables, which the A and B combinations draw from, and ONE slack variable per constraint,
    slack(i), which occurs in the C combination of constraint i and nowhere else.  C is chosen so that the row holds for ANY values of
    the shared variables once the slack is solved for (witness()), in three shapes by i % 3:
        [(slack, 1)]  ->  a b        [(0, k), (slack, 1)]  ->  a b - k        [(slack, q)], q != 0  ->  a b / q
    so one circuit has many satisfied witnesses, and a changed slack value breaks exactly its own row."""

    def __init__(self, zk, seed, n_constraints, num_inputs, num_aux):
        self.rng = np.random.default_rng(seed)
        self.num_inputs, self.n_shared, self.n_constraints = num_inputs, num_inputs + num_aux, n_constraints
        rng, n_shared = self.rng, self.n_shared

        def coeff():
            k = int(rng.integers(0, 10))
            return (1, 1, 1, R_ORDER - 1, R_ORDER - 1, 1 << int(rng.integers(1, 254)), 2, 0, self.uniform(), self.uniform())[k]

        def lc(i, which):                                   # the combinations of r1cs_cases.random_circuit
            length = int(rng.choice([0, 1, 1, 2, 2, 3, 3, 5, 9]))
            terms = [(int(rng.integers(0, n_shared)), coeff()) for _ in range(length)]
            if i % 7 == which:
                terms.append((0, coeff()))
            if i % 11 == which and terms:
                terms.append((terms[0][0], coeff()))
            if i % 13 == which:
                terms.append((int(rng.integers(0, n_shared)), 0))
            if i == 50 + which:
                terms = [(int(rng.integers(0, n_shared)), coeff()) for _ in range(70)]
            if i == 60 + which:
                terms = []
            return terms

        constraints = []
        for i in range(n_constraints):
            s = self.slack(i)
            c = ([(s, 1)], [(0, self.uniform()), (s, 1)], [(s, self.uniform() or 1)])[i % 3]
            constraints.append((lc(i, 0), lc(i, 1), c))
        self.circuit = zk.circom.CircomCircuit(num_inputs, num_aux + n_constraints, n_constraints, constraints)
        self.circuit.witness = self.witness()

    def uniform(self):
        return int.from_bytes(self.rng.bytes(40), "little") % R_ORDER

    def slack(self, i):
        return self.n_shared + i

    def witness(self):
        """a fresh satisfied witness: w[0] = 1, the shared values 0, 1, small, r - 1 and uniform, every slack solved for"""
        kinds = self.rng.integers(0, 10, size=self.n_shared)
        w = [1] + [1 if k < 2 else 0 if k < 4 else int(self.rng.integers(0, 256)) if k == 4 else R_ORDER - 1 if k == 5 else self.uniform()
                   for k in kinds[1:]]
        for i, (ca, cb, cc) in enumerate(self.circuit.constraints):
            p = sum(c * w[v] for v, c in ca) * sum(c * w[v] for v, c in cb) % R_ORDER
            if i % 3 == 0:
                w.append(p)
            elif i % 3 == 1:
                w.append((p - cc[0][1]) % R_ORDER)
            else:
                w.append(p * pow(cc[0][1], -1, R_ORDER) % R_ORDER)
        return w

    def break_witness(self, witness, rows):
        """a copy of `witness` that breaks exactly `rows`: each row's slack value plus one"""
        w = list(witness)
        for i in rows:
            w[self.slack(i)] = (w[self.slack(i)] + 1) % R_ORDER
        return w

    def break_coefficient(self, zk, rows):
        """a copy of the circuit (same witness) that breaks exactly `rows`: the coefficient of ONE in C plus one (a term of its own)"""
        constraints = list(self.circuit.constraints)
        for i in rows:
            a, b, c = constraints[i]
            constraints[i] = (a, b, c + [(0, 1)])
        return zk.circom.CircomCircuit(self.circuit.num_inputs, self.circuit.num_aux, self.n_constraints, constraints, list(self.circuit.witness))


def satisfied_circuit(zk, seed=5100, n_constraints=300, num_inputs=5, num_aux=61) -> Satisfied:
    return Satisfied(zk, seed, n_constraints, num_inputs, num_aux)


def row_values(circuit, witness, i):
    """(a, b, c) of constraint i as canonical ints"""
    return tuple(sum(c * witness[v] for v, c in lc) % R_ORDER for lc in circuit.constraints[i])


def failing_rows(circuit, witness):
    return [i for i in range(len(circuit.constraints)) if (lambda a, b, c: a * b % R_ORDER != c)(*row_values(circuit, witness, i))]


def verdict(a, b, c):
    """the big-int model of the check on canonical ints: (lowest failing row or -1, number of failing rows)"""
    bad = [i for i, (x, y, z) in enumerate(zip(a, b, c)) if x * y % R_ORDER != z]
    return (bad[0] if bad else -1, len(bad))
