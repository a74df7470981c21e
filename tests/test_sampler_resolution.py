"""CPU checks of the device sampler's mathematics (rfm_sample.hip), restated in NumPy:

* the windowed masked-rejection walk of the draws kernel gives NumPy's swap partners j_i;
* the parallel resolution of the first B shuffled entries from j reproduces
  ``RandomState(seed).shuffle(arange(N))[:B]``;
* the workspace query's arithmetic (12 N + 8 B bytes per epoch in flight) and its checks.

No GPU is needed: the library's host-only query is called, nothing is launched."""
import ctypes as C

import numpy as np
import pytest

from relevance_factorizationmachine_amd import _lib

MT_N = 624


def mask_for(x: int) -> int:
    return (1 << int(x).bit_length()) - 1


def draws_sequential(n: int, seed: int) -> np.ndarray:
    """j_i for i = n-1 .. 1 exactly as NumPy's legacy random_interval draws them."""
    bg = np.random.RandomState(seed)._bit_generator
    raw = bg.random_raw(3 * n + 1000)
    t, j = 0, np.zeros(n, np.int64)
    for i in range(n - 1, 0, -1):
        m = mask_for(i)
        while True:
            v = int(raw[t]) & m
            t += 1
            if v <= i:
                break
        j[i] = v
    return j


def draws_windowed(n: int, seed: int) -> np.ndarray:
    """The draws kernel's walk: windows of up to 64 outputs of one 624-word block, settled lanes
    taken by a ballot (the lanes below the first unsettled one), then the first unsettled lane on
    its own with its exact step.  Returns j and checks that every window makes progress."""
    bg = np.random.RandomState(seed)._bit_generator
    raw = bg.random_raw(3 * n + 2 * MT_N + 1000).astype(np.uint64)
    j = np.zeros(n, np.int64)
    cur, block, pos = n - 1, -MT_N, MT_N
    lanes = np.arange(64)
    while cur >= 1:
        if pos >= MT_N:
            block, pos = block + MT_N, 0
        avail = MT_N - pos
        vals = np.zeros(64, np.int64)
        vals[: min(avail, 64)] = raw[block + pos: block + pos + min(avail, 64)]
        mask = mask_for(cur)
        half = mask >> 1
        v = vals & mask
        fixed = (lanes < avail) & (lanes + half < cur)
        accept = fixed & (v + lanes <= cur)
        settled = accept | (fixed & (v > cur))
        a = int(np.argmin(settled)) if not settled.all() else 64
        assert a >= 1
        acc = np.flatnonzero(accept[:a])
        for rank, lane in enumerate(acc):
            j[cur - rank] = v[lane]
        cur -= len(acc)
        pos += a
        if a < 64 and a < avail and cur >= 1:
            va = int(vals[a]) & mask_for(cur)
            if va <= cur:
                j[cur] = va
                cur -= 1
            pos += 1
    return j


def first_b(n: int, b: int, j: np.ndarray) -> np.ndarray:
    """The resolve step: out[p] = g(succ(p)) or j_p, with M, the buckets and g as the kernels
    build them."""
    m = np.full(n, n, np.int64)
    steps = np.arange(n)
    sel = j != steps
    np.minimum.at(m, j[sel], steps[sel])
    buckets = {}
    for i in np.flatnonzero(j < b):
        buckets.setdefault(int(j[i]), []).append(int(i))
    out = np.empty(b, np.int64)
    for p in range(b):
        later = [i for i in buckets[int(j[p])] if i > p]
        if not later:
            out[p] = j[p]
            continue
        x = min(later)
        while m[x] != n:
            x = int(m[x])
        out[p] = x
    return out


def numpy_first_b(n: int, b: int, seed: int) -> np.ndarray:
    a = np.arange(n)
    np.random.RandomState(seed).shuffle(a)
    return a[:b]


CASES = [(1, 1, 0), (2, 1, 0), (2, 2, 3), (3, 3, 1), (5, 2, 7), (10, 3, 0), (63, 63, 4), (64, 17, 9),
         (65, 65, 2), (1000, 17, 5), (4096, 100, 11), (4097, 4097, 1), (3000, 1, 8), (5000, 5000, 2 ** 32 - 1)]


@pytest.mark.parametrize("n,b,seed", CASES)
def test_windowed_draws_match_numpy(n, b, seed):
    assert np.array_equal(draws_windowed(n, seed), draws_sequential(n, seed))


@pytest.mark.parametrize("n,b,seed", CASES)
def test_resolution_matches_numpy_shuffle(n, b, seed):
    assert np.array_equal(first_b(n, b, draws_windowed(n, seed)), numpy_first_b(n, b, seed))


def _workspace(n, b, g):
    out = C.c_int64(-1)
    rc = _lib.load().rfm_sample_batches_device_workspace(n, b, g, C.byref(out))
    return rc, out.value


@pytest.mark.parametrize("n,b,g", [(1, 1, 1), (1000, 17, 1), (1000, 1000, 3), (1_000_000, 65_536, 40),
                                   (2 ** 31 - 1, 2 ** 31 - 1, 2)])
def test_workspace_query(n, b, g):
    rc, got = _workspace(n, b, g)
    assert rc == _lib.RFM_OK
    assert got == g * (12 * n + 8 * b)


def test_workspace_query_checks():
    rc, _ = _workspace(10, 11, 1)
    assert rc == _lib.RFM_ERR_BAD_ARG
    assert _lib.last_error() == "Cannot sample 11 out of arrays with dim 10 when replace is False"
    for n, b, g in [(0, 1, 1), (2 ** 31, 1, 1), (10, 0, 1), (10, 5, 0)]:
        assert _workspace(n, b, g)[0] == _lib.RFM_ERR_BAD_ARG
