"""LQProblem.set_batch_weights: argument validation and index computation, on the host alone (no library call is made
for a wrong shape; for a right one the call handed to set_batch_params is checked)."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def ocs():
    import __graft_entry__ as g
    return g.load_package()


class Recorder:
    def __init__(self, ocs, nS, nC):
        self.p = ocs.LQProblem.__new__(ocs.LQProblem)   # no handle: nothing below may reach the library
        self.p.nS, self.p.nC, self.p.nAug = nS, nC, nS + 1
        self.calls = []
        self.p.set_batch_params = lambda index, values: self.calls.append((list(index), values))


@pytest.mark.parametrize("q,rdiag", [
    (np.ones((4, 6)), None),            # q has nS = 5 rows
    (np.ones(5), None),                 # not two-dimensional
    (None, np.ones((3, 6))),            # rdiag has nC = 2 rows
    (np.ones((5, 6)), np.ones((2, 7))),  # disagreeing batch sizes
    (np.ones((5, 0)), None),            # empty batch
    (np.ones((6, 5)), np.ones((6, 2))),  # transposed
])
def test_wrong_shapes_raise_before_any_library_call(ocs, q, rdiag):
    r = Recorder(ocs, 5, 2)
    with pytest.raises(ValueError):
        r.p.set_batch_weights(q, rdiag)
    assert r.calls == []


def test_indices_and_values(ocs):
    nS, nC, batch = 5, 2, 3
    w0 = 1 + nS * nS + nS * nC
    q, rd = np.arange(nS * batch, dtype=float).reshape(nS, batch), -np.arange(nC * batch, dtype=float).reshape(nC, batch)
    r = Recorder(ocs, nS, nC)
    r.p.set_batch_weights(q, rd)
    r.p.set_batch_weights(None, rd)
    r.p.set_batch_weights(q)
    r.p.set_batch_weights()
    (i0, v0), (i1, v1), (i2, v2), (i3, v3) = r.calls
    assert i0 == list(range(w0, w0 + nS + nC)) and np.array_equal(v0, np.vstack([q, rd]))
    assert i1 == list(range(w0 + nS, w0 + nS + nC)) and np.array_equal(v1, rd)
    assert i2 == list(range(w0, w0 + nS)) and np.array_equal(v2, q)
    assert i3 == [] and v3 is None
    assert w0 + nS + nC == 1 + nS * nS + nS * nC + nS + nC   # the end of [r | A | Bu | q | rdiag]
