"""CPU: what the scan tools share in buglab/controllers/_batching.py -- `RunColumns`, the one owner of run-long result buffers
(alignment, contiguity and the growth copy along each column's own sample axis, from capacity 1), and `predictions_in_order`,
the one walk over `model.predict` (input order, the rejected ones, a foreign datapoint)."""
import numpy as np
import pytest
import torch

from buglab.controllers import _batching as Bt
from buglab.controllers._batching import SAMPLES, RunColumns

# an odd number of 4-byte cells sits in front of an fp64 column at odd capacities
SPEC = (("score", "float64", (SAMPLES, 3)), ("node", "int32", (SAMPLES, 3)), ("rank", "int32", (2, SAMPLES)),
        ("logprob", "float32", (SAMPLES,)), ("objective", "float64", (SAMPLES,)))
DTYPES = {"float64": np.float64, "float32": np.float32, "int32": np.int32}


def _expected(column: int, n: int) -> np.ndarray:
    """the first n samples of a column: a value per (column, sample index, inner index), exact in every dtype"""
    name, dtype, shape = SPEC[column]
    axis = shape.index(SAMPLES)
    index = np.indices([n if s == SAMPLES else s for s in shape])
    values = 1000 * (column + 1) + 10 * index[axis] + (index[1 - axis] if len(shape) == 2 else 0)
    return (values + (0.25 if dtype != "int32" else 0)).astype(DTYPES[dtype])


def _check_views(cols: RunColumns, n: int) -> None:
    for c, (name, dtype, shape) in enumerate(SPEC):
        view = cols[name]
        assert view.data_ptr() % 8 == 0 and view.is_contiguous(), name
        assert tuple(view.shape) == tuple(cols.capacity if s == SAMPLES else s for s in shape)
        got = view.narrow(shape.index(SAMPLES), 0, n).numpy()
        assert got.tobytes() == _expected(c, n).tobytes(), name  # the earlier samples, bit for bit


def test_run_columns_grow_from_capacity_one():
    cols = RunColumns("cpu", 1, SPEC)
    capacity = 1
    for B in (3, 0, 5, 1):
        n = cols.reserve(B)
        if n + B > capacity:
            capacity = max(2 * capacity, n + B)
        assert cols.capacity == capacity and cols.n == n + B
        _check_views(cols, n)
        for c, (name, _, shape) in enumerate(SPEC):
            axis = shape.index(SAMPLES)
            cols[name].narrow(axis, n, B).copy_(torch.from_numpy(_expected(c, n + B)).narrow(axis, n, B))
        _check_views(cols, n + B)
    assert cols.n == 9 and cols.capacity == 16
    host, device = cols.to_host(), cols.device_columns()
    for c, (name, dtype, shape) in enumerate(SPEC):
        want = _expected(c, 9)
        assert host[name].dtype == want.dtype and host[name].shape == want.shape and host[name].tobytes() == want.tobytes()
        assert device[name].device.type == "cpu" and tuple(device[name].shape) == want.shape
        assert device[name].numpy().dtype == want.dtype and np.array_equal(device[name].numpy(), want)


def test_run_columns_without_samples():
    cols = RunColumns("cpu", 4, SPEC)
    assert cols.reserve(0) == 0 and cols.capacity == 4
    host, device = cols.to_host(), cols.device_columns()
    for name, dtype, shape in SPEC:
        want = tuple(0 if s == SAMPLES else s for s in shape)
        assert host[name].shape == want and host[name].dtype == DTYPES[dtype]
        assert tuple(device[name].shape) == want and device[name].numpy().dtype == DTYPES[dtype]


class _Stub:
    """a model whose `predict` passes over the inputs at `skip` and, with `foreign`, yields an object it was not given"""

    def __init__(self, skip, foreign=False):
        self.skip, self.foreign = set(skip), foreign

    def predict(self, data, nn, device, parallelize):
        for i, point in enumerate(data):
            if i not in self.skip:
                yield (dict(point) if self.foreign else point), {-1: float(i)}, [float(i)]


def test_predictions_in_order_reports_what_predict_passed_over():
    points = [{"id": i} for i in range(10)]
    skip = (0, 4, 5, 6, 9)  # the first, a middle run and the last
    events = []
    found = Bt.predictions_in_order(_Stub(skip), None, ((p, 100 + i) for i, p in enumerate(points)), "cpu", False,
                                    lambda tag: events.append(("rejected", tag)), "stub: predict")
    for tag, point, location_logprobs, rewrite_logprobs in found:
        assert point is points[tag - 100] and location_logprobs == {-1: float(tag - 100)} and rewrite_logprobs == [float(tag - 100)]
        events.append(("yielded", tag))
    assert [tag for _, tag in events] == [100 + i for i in range(10)]  # together: the input order
    assert [tag - 100 for kind, tag in events if kind == "rejected"] == list(skip)


def test_predictions_in_order_refuses_a_foreign_datapoint():
    points = [{"id": i} for i in range(3)]
    rejected = []
    with pytest.raises(RuntimeError, match="^stub: predict yielded a datapoint it was not given$"):
        list(Bt.predictions_in_order(_Stub((), foreign=True), None, ((p, i) for i, p in enumerate(points)), "cpu", False, rejected.append,
                                     "stub: predict"))
