"""The host code that every fit driver shares (evaluate.runs, evaluate.SlotLoop): no GPU needed."""
import numpy as np
import pytest
import torch

from relevance_factorizationmachine_amd import evaluate

CHUNK = 5


@pytest.mark.parametrize("first,count,limit,bound", [
    (0, 0, lambda at: 3, 3),
    (7, 0, lambda at: 3, 3),
    (0, 1, lambda at: 3, 3),
    (4, 1, lambda at: 1, 1),
    (3, 9, lambda at: 1, 1),                         # a limit of 1: one run per iteration
    (3, 9, lambda at: 100, 100),                     # a limit larger than count: one run
    (0, 16, lambda at: CHUNK - at % CHUNK, CHUNK),   # score slots, first on a chunk edge
    (7, 16, lambda at: CHUNK - at % CHUNK, CHUNK),   # ... and inside a chunk
    (16, 64, lambda at: CHUNK - at % CHUNK, CHUNK),  # (the second id chunk of a BatchIdStream)
    (9, 1, lambda at: CHUNK - at % CHUNK, CHUNK),
])
def test_runs_cover_every_iteration_once_within_their_limits(first, count, limit, bound):
    got = list(evaluate.runs(first, count, limit))
    at = first
    for start, n in got:
        assert start == at and 1 <= n <= limit(start)   # contiguous, not empty, within the limit
        if bound == CHUNK:
            assert start // CHUNK == (start + n - 1) // CHUNK  # never across a multiple of the chunk
        at += n
    assert at == first + count
    assert [e for start, n in got for e in range(start, start + n)] == list(range(first, first + count))
    if count == 0:
        assert got == []
    if bound == 1:
        assert len(got) == count
    if bound == 100:
        assert got == [(first, count)]


class _Rt:
    """A runtime whose device is the host: torch CPU tensors, nothing to wait for."""

    def __init__(self):
        self.syncs = 0

    def sync(self):
        self.syncs += 1

    def empty(self, shape, dtype):
        return torch.zeros(shape, dtype=dtype)


class _Loop(evaluate.SlotLoop):
    def __init__(self, rt, n_epochs, per_iter):
        super().__init__(rt, n_epochs, per_iter)
        self.asked = []

    def _resolve(self, flagged):
        self.asked.append(list(flagged))
        return {e: 1000.0 + e for e in flagged}


def test_flush_resolves_the_flagged_iterations_of_a_chunk_in_one_call(monkeypatch):
    monkeypatch.setattr(evaluate.EvalLoop, "CHUNK_BYTES", 3 * 40)  # (read at construction time)
    rt = _Rt()
    loop = _Loop(rt, 8, 40)
    assert loop.chunk == 3 and [loop.room(e) for e in range(5)] == [3, 2, 1, 3, 2]
    # iteration e leaves the value e; 1, 2 and 6 have tie-order dependent users (e + 1 of them)
    table = np.array([[float(e), float(e + 1) if e in (1, 2, 6) else 0.0] for e in range(8)])
    loop.out.copy_(torch.from_numpy(table))
    loop.ran(0, 2)
    assert loop.values == [] and rt.syncs == 0           # the chunk is not complete: nothing is read
    loop.ran(2, 1)
    assert loop.values == [0.0, 1001.0, 1002.0] and loop.asked == [[1, 2]] and rt.syncs == 1
    loop.ran(3, 3)
    assert loop.asked == [[1, 2], []] and rt.syncs == 2   # (every flush asks once: the exchange pairs up)
    assert loop.finish(8) == [0.0, 1001.0, 1002.0, 3.0, 4.0, 5.0, 1006.0, 7.0]
    assert loop.asked == [[1, 2], [], [6]] and rt.syncs == 3
    assert (loop.host_calls, loop.host_users) == (3, 2 + 3 + 7)
    assert loop.finish(8) is loop.values and rt.syncs == 3  # nothing left to flush
