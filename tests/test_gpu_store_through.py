"""What a launch of the FM step leaves for the NEXT launch on the stream -- Q rows, slot marks, hot-sum
slabs, updated rows of V, gradient rows -- where no host synchronisation lies between the two, and the
16-byte pairs the forward writes its hot-sum slabs in.  Needs an MI355X: ``pytest -m gpu``.

A  rfm_fm_train of six iterations in ONE call (launches back to back on the stream) against six calls
   of one iteration, each followed by a synchronise and a read-back of w0, w and V.  Both run the same
   kernels on the same numbers: where every sum of a step has a fixed order (hot_min_count -1 or -2,
   or several chunks of factors per lane) the parameters are equal bit for bit, in the default mode
   (hot sums by LDS float atomics: arrival order) they agree to 1e-13 of the largest parameter, the
   bound test_gpu_grad_forms.py holds two runs of three steps to (the learning rates here move a
   parameter by far less than its size, so a sum's last bits reach the result scaled down).
B  The slab store: a row of k + 2 doubles goes out as (k + 2) / 2 pairs when k is even, one double at
   a time when it is odd.  Dense gradients and record lists of a whole small log (several forward
   workgroups) and of a five-row shard (one workgroup; two at k = 128), with 1 and with 7 hot columns, against the
   long-double oracle of grad_forms_common.py under its own comparisons and tolerances."""
import functools

import numpy as np
import pytest

import forward_rows_common as fr
import grad_forms_common as gf
from conftest import rel_err

pytestmark = pytest.mark.gpu

BIG, SMALL = 1024, 256
N_ITERS = 6


@pytest.fixture(scope="module")
def rt():
    from relevance_factorizationmachine_amd import runtime
    return runtime.Runtime.get()


def _chunked(k):
    """Several chunks of factors per lane (include/rfm_hip.h: more than 128 factors, or an odd count
    above 64): no hot class, every sum in a fixed order."""
    return k > 128 or (k % 2 == 1 and k > 64)


def _fixed_order(k, hot):
    return hot in (-1, -2) or _chunked(k)


# --------------------------------------------------------------------------
# A. launches back to back against one step at a time
# --------------------------------------------------------------------------
def _train(rt, dev, params, ids, lr):
    """rfm_fm_train over the batches ids [n_iters, batch]: steps only, no loss forwards."""
    from relevance_factorizationmachine_amd import _lib
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    n_iters, batch = ids.shape
    d_ids = rt.upload(ids.reshape(-1))
    _lib.check(rt.lib.rfm_fm_train(rt.ctx, dev.plan.handle, *dev.log_ptrs(), d_ids.data_ptr(), batch, n_iters,
                                   *params.ptrs(), lr, None, None, None, None, None, 0, fr.EPS, None, None))
    rt.sync()


def _batches(seed, n_rows, batch):
    """Distinct ids within an iteration, another draw each iteration."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(n_rows)[:batch] for _ in range(N_ITERS)]).astype(np.int32)


def _check_back_to_back(rt, log, theta, k, hot, ids, lr, check_plan):
    import torch
    n_rows = log["features"].shape[0]
    batch = ids.shape[1]
    assert batch <= n_rows
    # six iterations in one call
    dev = gf.DeviceLog(rt, log, k, batch, hot)
    try:
        check_plan(dev)
        once = gf.Params(rt, *theta)
        _train(rt, dev, once, ids, lr)
        got = once.host()
    finally:
        dev.close()
    # one iteration per call on a plan of its own, the parameters read back after each
    dev = gf.DeviceLog(rt, log, k, batch, hot)
    try:
        stepwise = gf.Params(rt, *theta)
        before = stepwise.host()
        for it in range(N_ITERS):
            _train(rt, dev, stepwise, ids[it: it + 1], lr)
            torch.cuda.synchronize()
            want = stepwise.host()
            assert all(np.isfinite(a).all() for a in want), it
            assert not np.array_equal(want[2], before[2]), f"iteration {it} left V as it was"
            before = want
    finally:
        dev.close()
    for name, a, b in zip(("w0", "w", "V"), got, want):
        if _fixed_order(k, hot):
            np.testing.assert_array_equal(a, b, err_msg=name)
        else:
            err = rel_err(a, b)
            print(f"{name}: max |one call - six calls| / max |.| = {err:.3g}")
            assert err < 1e-13, (name, err)


@functools.lru_cache(maxsize=None)
def _small_log():
    """1 500 rows x 140 columns, two columns in every row (hot at a batch of 500 in the default and -2
    modes), the others at 4 %: 20 expected entries per batch, every one below the hot threshold of 32."""
    log = gf._random_log(np.random.default_rng(77), 1500, 140, 0.04, 2)
    counts = log["features"].getnnz(axis=0)
    assert (counts[:2] == 1500).all() and counts[2:].max() * 500 < 32 * 1500
    return log


HOT_MODES = (0, -1, -2)


@pytest.mark.parametrize("hot", HOT_MODES)
def test_back_to_back_many_rows_shape(rt, hot):
    """k = 32 at the smallest batch of the 1 024-thread forward shape; a log of 56 columns, every one
    of them frequent: the hot class in the default and -2 modes, long column lists without one."""
    k = 32
    batch = fr.many_rows_minimum(rt, k, True)
    geo = fr.forward_geometry(rt, batch, k, True)
    assert geo["block"] == BIG and fr.forward_geometry(rt, batch - 1, k, True)["block"] == SMALL
    lpr = geo["lpr"]
    # (the log of test_gpu_forward_rows.py's many-rows gradient case: made once per process)
    log, theta, _ = fr.case(k, batch + geo["trip"] + 1, (), (), lpr, 21, None, 8, 0)

    def check_plan(dev):
        info = dev.plan.info()
        assert (info["hot_columns"] > 0) == (hot != -1), info
        assert info["forward_workgroups"] == geo["grid"] > 1

    ids = _batches(k + hot, log["features"].shape[0], batch)
    _check_back_to_back(rt, log, theta, k, hot, ids, 2.0 ** -16, check_plan)


@pytest.mark.parametrize("hot", HOT_MODES)
@pytest.mark.parametrize("k", [32, 9, 34, 2])
def test_back_to_back_one_row_shape(rt, k, hot):
    """B = 500: k = 32; k = 9 (one factor per lane: every store plain); k = 34 and k = 2 (the
    smallest even rows: slab rows of 36 and of 4 doubles)."""
    log = _small_log()
    n_rows, n = log["features"].shape
    batch = 500
    assert fr.forward_geometry(rt, batch, k, True)["block"] == SMALL

    def check_plan(dev):
        assert dev.plan.info()["hot_columns"] == (0 if hot == -1 else 2)

    _check_back_to_back(rt, log, gf.perturbed_init(k, n, k), k, hot, _batches(k + hot, n_rows, batch), 2.0 ** -12,
                        check_plan)


def test_back_to_back_chunk_form(rt):
    """k = 300 at B = 500: three chunks of factors, dealt to different workgroups of the gradient
    launch; no hot class."""
    k = 300
    log = _small_log()
    n_rows, n = log["features"].shape
    assert _chunked(k) and fr.forward_geometry(rt, 500, k, True)["block"] == SMALL

    def check_plan(dev):
        assert dev.plan.info()["hot_columns"] == 0

    _check_back_to_back(rt, log, gf.perturbed_init(k, n, k), k, 0, _batches(k, n_rows, 500), 2.0 ** -12, check_plan)


@pytest.mark.parametrize("k,hot", [c for c in gf.CASES_B if c[0] in (128, 300)],
                         ids=lambda v: str(v))
def test_back_to_back_split_column(rt, k, hot):
    """The short split-column cases of test_gpu_grad_forms.py at k = 128 (fm_finalize_kernel) and
    k = 300 (fm_finalize_chunk_kernel): every iteration takes the whole log, so the partial rows of
    the dense column go from the gradient launch to the finalize launch every step."""
    n_rows = gf.full_batch_workgroup_slots(k) + 37
    log, theta, _, _ = gf.split_case(k, n_rows, 60, 1, 7 * k + len("short"))

    def check_plan(dev):
        info = dev.plan.info()
        assert info["split_columns"] >= 1 and info["hot_columns"] == 0, info

    _check_back_to_back(rt, log, theta, k, hot, _batches(k, n_rows, n_rows), 2.0 ** -10, check_plan)


# --------------------------------------------------------------------------
# B. the slab store in pairs
# --------------------------------------------------------------------------
SLAB_ROWS, SLAB_COLS = 400, 120


@functools.lru_cache(maxsize=None)
def _slab_case(k, n_hot):
    """400 rows x 120 columns: ``n_hot`` columns in every row, the others at 3 % (12 entries each on
    average, the threshold of the hot class is 32); parameters, the whole log in shuffled order, a
    five-row shard and the oracle gradients of both: computed once, shared by the hot modes."""
    rng = np.random.default_rng(1000 * k + n_hot)
    log = gf._random_log(rng, SLAB_ROWS, SLAB_COLS, 0.03, n_hot)
    counts = log["features"].getnnz(axis=0)
    assert (counts[:n_hot] == SLAB_ROWS).all() and counts[n_hot:].max() < 32
    theta = gf.perturbed_init(k + n_hot, SLAB_COLS, k)
    full = rng.permutation(SLAB_ROWS).astype(np.int32)
    shard = np.array([SLAB_ROWS - 1, 3, 0, SLAB_ROWS // 3, 17], dtype=np.int32)
    return log, theta, full, shard, gf.grad_oracle(log, full, *theta), gf.grad_oracle(log, shard, *theta)


# (k = 128 with 7 hot columns: 7 * 65 pairs, more than the 256 threads of a workgroup store in one trip)
SLAB_CASES = [(k, h) for k in (2, 9, 32, 34) for h in (1, 7)] + [(128, 7)]


@pytest.mark.parametrize("hot", [0, -2])
@pytest.mark.parametrize("k,n_hot", SLAB_CASES, ids=[f"k{k}-H{h}" for k, h in SLAB_CASES])
def test_slab_rows_in_pairs(rt, k, n_hot, hot):
    log, theta, full, shard, o_full, o_shard = _slab_case(k, n_hot)
    dev = gf.DeviceLog(rt, log, k, len(full), hot)
    try:
        assert dev.plan.info()["hot_columns"] == n_hot
        np.testing.assert_array_equal(np.sort(dev.plan.hot_columns()), np.arange(n_hot))
        # the whole log: several forward workgroups (slabs); the shard: one
        assert fr.forward_geometry(rt, len(full), k, True)["grid"] > 1
        one = fr.forward_geometry(rt, len(shard), k, True)
        assert one["grid"] == -(-len(shard) // one["trip"]) and (one["grid"] == 1 or k == 128)
        gf.check_all_forms(dev, gf.Params(rt, *theta), full, shard, o_full, o_shard, hot == -2)
    finally:
        dev.close()
