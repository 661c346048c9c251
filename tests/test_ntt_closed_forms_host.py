"""The closed forms of tests/ntt_edge_forms.py against the CPU oracle's domain operations, every pattern and operation at 2^1 .. 2^10: this
fixes omega, the coset generator and the scaling conventions of the forms before tests/test_gpu_ntt_edges.py holds the device to them."""
import numpy as np
import pytest

import ntt_edge_forms as E
import oracle_lib as O


@pytest.mark.parametrize("op", E.OPS)
@pytest.mark.parametrize("log_n", range(1, 11))
def test_closed_forms_match_the_oracle(log_n, op):
    cs = E.cases(log_n, op)
    names = [name for name, _, _ in cs]
    assert len(set(names)) == len(names)
    for what in ("all zero", "all c", "all one", "c at 0", "c at %d" % ((1 << log_n) - 1), "c on even, 0 on odd", "c on even, 1 on odd", "tone %d" % ((1 << log_n) // 2)):
        assert any(n.startswith(what) for n in names), (what, names)
    if op == "coset_fft":
        assert any(n.endswith(", raw") for n in names)
    for name, a, want in cs:
        assert a.shape == want.shape == (1 << log_n, 4)
        assert np.array_equal(O.fr_domain_op(a, log_n, op).reshape(-1, 4), want), (log_n, op, name)


def test_the_inputs_are_canonical_and_reach_the_largest_word():
    import bn254_model as M

    for op in E.OPS:
        for name, a, want in E.cases(6, op):
            for arr in (a, want):
                vals = [M.from_limbs([int(w) for w in row]) for row in arr]
                assert max(vals) < M.R_ORDER, (op, name)
    fft = dict((n, a) for n, a, _ in E.cases(6, "fft"))
    assert M.from_limbs([int(w) for w in fft["all c"][5]]) == M.R_ORDER - 1
