"""The gradient forms of the FM step -- rfm_fm_grad, rfm_fm_grad_rows, rfm_fm_apply,
rfm_fm_apply_rows, rfm_fm_reduce_rows, rfm_fm_set_rows: what the data-parallel fit is built from --
at every (lanes per row, vector width, chunks per lane) class of the kernels, in every hot mode, with
split columns of both forms, and at the edges of the record list.  Needs an MI355X: ``pytest -m gpu``.

Dense gradients are held to the long-double oracle of grad_forms_common.py, element by element:
|got - want| <= 1e-11 * S, S the sum of the absolute values of the terms of that element's sum (the
derivation is in that module).  Records are held to the dense gradient: bit for bit where every sum
has a fixed order (hot_min_count -1 or -2, or several chunks per lane), 1e-13 norm-wise otherwise."""
import functools

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import grad_forms_common as gf
from conftest import rel_err

pytestmark = pytest.mark.gpu

LD = np.longdouble
K_SHORT_SPLIT = 8  # kShortSplit: a split column of up to this many partial rows takes the short form


@pytest.fixture(scope="module")
def rt():
    from relevance_factorizationmachine_amd import runtime
    return runtime.Runtime.get()


CLASS_OF = gf.CLASS_OF
_class_id, _chunked, _fixed_order = gf.class_id, gf.chunked, gf.fixed_order
_check_all_forms, _oracle = gf.check_all_forms, gf.grad_oracle


# --------------------------------------------------------------------------
# A. the shape classes x the hot modes
# --------------------------------------------------------------------------
EMPTY_ROWS = (5, 700, 1499)
SHARD = np.array([11, 5, 1200, 42, 977], dtype=np.int32)  # row 5 is empty


@functools.lru_cache(maxsize=None)
def _log_a(small):
    """About 1 500 rows x 140 columns (750 x 70 for the largest factor counts, whose oracle is the
    slow part): two dense columns, frequent columns, rare columns (a quarter of the frequent ones'
    entries: below the default hot threshold of 32 per batch), columns nobody touches, empty rows."""
    n_rows, n_cols = (750, 70) if small else (1500, 140)
    rng = np.random.default_rng(2024 + small)
    log = gf._random_log(rng, n_rows, n_cols, 0.05 if not small else 0.1, 2)
    D = log["features"].toarray()
    rare = np.arange(n_cols // 2, n_cols)
    D[:, rare] *= rng.random((n_rows, len(rare))) < 0.25
    D[:, [17, n_cols // 2 + 3, n_cols - 1]] = 0.0
    D[[r % n_rows for r in EMPTY_ROWS], :] = 0.0
    log["features"] = csr_matrix(D)
    return log


@functools.lru_cache(maxsize=None)
def _case_a(k):
    """Log, parameters and the two oracle gradients of a factor count: computed once, shared by the
    hot modes, never modified."""
    log = _log_a(k >= 500)
    n_rows, n = log["features"].shape
    w0, w, V = gf.perturbed_init(k, n, k)
    full = np.random.default_rng(k).permutation(n_rows).astype(np.int32)
    shard = SHARD % n_rows
    assert log["features"][int(shard[1])].nnz == 0
    return log, (w0, w, V), full, shard, _oracle(log, full, w0, w, V), _oracle(log, shard, w0, w, V)


CASES_A = [(k, hot) for k in sorted(CLASS_OF) if k != 33 for hot in ((0,) if _chunked(k) else (0, -1, -2, 4))]


@pytest.mark.parametrize("k,hot", CASES_A, ids=[f"{_class_id(k)}-hot{hot}" for k, hot in CASES_A])
def test_gradient_forms_at_every_shape_class(rt, k, hot):
    log, theta, full, shard, o_full, o_shard = _case_a(k)
    dev = gf.DeviceLog(rt, log, k, len(full), hot)
    try:
        assert dev.plan.layout()["lanes_per_row"] == CLASS_OF[k][0]
        n_hot = dev.plan.info()["hot_columns"]
        # the class the case is meant for is really there (-2 at these batches: every single-chunk k)
        assert (n_hot > 0) == (hot != -1 and not _chunked(k)), n_hot
        if hot == 0 and n_hot:
            assert dev.plan.info()["hot_columns"] < dev.n  # the rare columns stay in the sparse class
        _check_all_forms(dev, gf.Params(rt, *theta), full, shard, o_full, o_shard, _fixed_order(k, hot))
    finally:
        dev.close()


# --------------------------------------------------------------------------
# B. split columns (a column longer than a workgroup's slots) in gradient mode
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _workgroup_slots(k):
    """Slots of a workgroup at batch = n_rows: it depends on the factor count alone; read from a
    plan of a small log through the public calls."""
    from relevance_factorizationmachine_amd import runtime
    rng = np.random.default_rng(1)
    dev = gf.DeviceLog(runtime.Runtime.get(), gf._random_log(rng, 64, 6, 0.3), k, 64, -1)
    try:
        assert dev.geometry()["BC"] == gf.full_batch_workgroup_slots(k)
        return dev.geometry()["BC"]
    finally:
        dev.close()


# the smallest row counts that reach the form: one workgroup's slots + a few rows -> 2 partial rows
# (short form), 8 workgroups' + a few -> 9 (long form).  At 4 lanes per row (k = 8) a workgroup has
# 4 096 slots: the long form needs about 33 000 rows, inside the 40 000 the tolerance is derived for.
CASES_B = gf.CASES_B
STEP_LR = 2.0 ** -3  # an update the size of the parameters


@pytest.mark.parametrize("form", ["short", "long"])
@pytest.mark.parametrize("k,hot", CASES_B, ids=[f"{_class_id(k)}-hot{hot}" for k, hot in CASES_B])
def test_split_columns_in_gradient_mode(rt, k, hot, form):
    bc = _workgroup_slots(k)
    n_rows = (bc if form == "short" else K_SHORT_SPLIT * bc) + 37
    assert n_rows <= gf.GRAD_TOL_ROWS
    log, theta, full, shard = gf.split_case(k, n_rows, 24 if n_rows > 5000 else 60, 1, 7 * k + len(form))
    dev = gf.DeviceLog(rt, log, k, n_rows, hot)
    try:
        assert dev.geometry()["BC"] == bc
        parts = dev.partial_rows(0)
        assert (2 <= parts <= K_SHORT_SPLIT) if form == "short" else parts > K_SHORT_SPLIT, parts
        info = dev.plan.info()
        assert info["split_columns"] >= 1 and info["hot_columns"] == 0
        o_full = _oracle(log, full, *theta)
        _check_all_forms(dev, gf.Params(rt, *theta), full, shard, o_full, _oracle(log, shard, *theta), True)
        # ... and in place: one step on the full batch against theta - lr * g, element by element
        # (grad_forms_common.step_bound); the split column's row goes through the finalize launch
        params = gf.Params(rt, *theta)
        gf.step(dev, full, params, STEP_LR)
        got = params.host()
        assert not np.array_equal(got[2][0], theta[2][0])  # the split column moved
        for name, ratio in zip(("w0", "w", "V"), gf.step_excess(got, theta, o_full, STEP_LR, n_rows)):
            print(f"{name}: worst |got - (theta - lr g)| / bound = {float(ratio.max()):.3g}")
            assert (ratio <= 1).all(), (name, np.argwhere(ratio > 1)[:5], float(ratio.max()))
    finally:
        dev.close()


def test_hot_class_overflow_leaves_dense_columns_split(rt):
    """More dense columns than the hot class takes (k = 64, default mode): some dense columns are
    summed on chip and some are split columns in the same step."""
    k = 64
    hot_cap = min(160, (56 << 10) // ((k + 2) * 8))
    bc = _workgroup_slots(k)
    n_rows, n_cols, dense = bc + 37, 150, hot_cap + 7
    assert dense < n_cols
    log, theta, full, shard = gf.split_case(k, n_rows, n_cols, dense, 64)
    dev = gf.DeviceLog(rt, log, k, n_rows, 0)
    try:
        info = dev.plan.info()
        assert info["hot_columns"] == hot_cap and info["split_columns"] == dense - hot_cap
        assert 2 <= dev.partial_rows(dense - 1) <= K_SHORT_SPLIT
        _check_all_forms(dev, gf.Params(rt, *theta), full, shard, _oracle(log, full, *theta),
                         _oracle(log, shard, *theta), False)
    finally:
        dev.close()


# --------------------------------------------------------------------------
# C. the forms agree with the step, interleaved on one plan
# --------------------------------------------------------------------------
def _apply_dense(rt, dev, ids, params, lr):
    from relevance_factorizationmachine_amd import _lib
    _, d_grad = gf.dense_grad(dev, ids, params)
    _lib.check(rt.lib.rfm_fm_apply(rt.ctx, *params.ptrs(), d_grad.data_ptr(), dev.n, dev.k, lr))
    rt.sync()


def _apply_records(rt, dev, ids, params, lr):
    from relevance_factorizationmachine_amd import _lib
    rec = gf.grad_rows(dev, ids, params, dev.n)
    _lib.check(rt.lib.rfm_fm_apply_rows(rt.ctx, rec.d_rows.data_ptr(), rec.d_n.data_ptr(), dev.n,
                                        rec.d_gw0.data_ptr(), *params.ptrs(), dev.n, dev.k, lr))
    rt.sync()
    return rec


@pytest.mark.parametrize("hot", [0, -1])
@pytest.mark.parametrize("k", [16, 65, 400])
def test_forms_interleaved_on_one_plan_equal_the_step(rt, k, hot):
    """step, grad + apply and grad_rows + apply_rows, one batch each, on ONE plan, in the three
    rotations of that order: every form runs at both parities of the chunked bitmap and after each
    of the others' stamps.  Each rotation against three steps on a fresh plan."""
    log = _log_a(False)
    n_rows, n = log["features"].shape
    batch, lr = 400, 1e-4
    rng = np.random.default_rng(k + hot)
    batches = [rng.permutation(n_rows)[:batch].astype(np.int32) for _ in range(3)]
    theta = gf.perturbed_init(k, n, k)
    fresh = gf.DeviceLog(rt, log, k, batch, hot)
    ref = gf.Params(rt, *theta)
    for b in batches:
        gf.step(fresh, b, ref, lr)
    ref_w0, ref_w, ref_V = ref.host()
    fresh.close()
    assert rel_err(ref_V, theta[2]) > 1e-6  # the three steps moved the parameters

    dev = gf.DeviceLog(rt, log, k, batch, hot)
    hot_cols = dev.plan.hot_columns()
    assert (len(hot_cols) > 0) == (hot == 0 and not _chunked(k))
    try:
        for rot in range(3):
            params = gf.Params(rt, *theta)
            for i, b in enumerate(batches):
                form = (i + rot) % 3
                if form == 0:
                    gf.step(dev, b, params, lr)
                elif form == 1:
                    _apply_dense(rt, dev, b, params, lr)
                else:
                    # an empty shard between two real calls: no records, g_w0 exactly zero ...
                    none = gf.grad_rows(dev, np.array([], dtype=np.int32), params, dev.n)
                    assert none.count == 0 and none.gw0 == 0.0
                    none.assert_rest_untouched()
                    # ... and the next call's list is that call's own
                    rec = _apply_records(rt, dev, b, params, lr)
                    cols = rec.filled()[:, 0].astype(np.int64)
                    np.testing.assert_array_equal(cols, np.union1d(np.unique(log["features"][b].indices), hot_cols))
            w0, w, V = params.host()
            assert rel_err(V, ref_V) < 1e-13 and rel_err(w, ref_w) < 1e-13 and rel_err(w0, ref_w0) < 1e-13, rot
    finally:
        dev.close()


# --------------------------------------------------------------------------
# D. the edges of the record list (count -> scan -> gather, owner-range bounds)
# --------------------------------------------------------------------------
CHUNK = 2048  # columns per workgroup of the compaction


def _touched_sets(n):
    """Named column sets of a log of n columns; the groups of rows of `_list_log` touch one each."""
    rng = np.random.default_rng(n)
    last_chunk = (n - 1) // CHUNK
    sets = {}
    # first and last column, a few between: every chunk between them is empty or nearly so
    some = rng.choice(n, size=min(n, 40), replace=False)
    sets["ends"] = np.union1d([0, n - 1], some[: max(0, min(len(some), n // 2))])
    sets["last"] = np.array([n - 1])
    # a chunk fully touched: the second one where there are three (empty chunks on both sides), with
    # another past the 256th where there are that many; else the first (or what there is of it)
    first = CHUNK if n >= 3 * CHUNK else 0
    full = [np.arange(first, min(first + CHUNK, n))]
    if last_chunk > 256:
        full.append(np.arange(256 * CHUNK, 257 * CHUNK))
    sets["full_chunk"] = np.concatenate(full)
    near = np.concatenate([np.arange(0, min(n, 2 * CHUNK + 100)), np.arange(max(0, n - 100), n)])
    near = np.unique(near)
    sets["evens"], sets["odds"] = near[near % 2 == 0], near[near % 2 == 1]  # disjoint, interleaved
    return {name: np.asarray(s, dtype=np.int64) for name, s in sets.items() if len(s)}


@functools.lru_cache(maxsize=None)
def _list_log(n):
    """Rows of one to three entries on chosen columns: group g's rows hold exactly the set g."""
    rng = np.random.default_rng(3 * n + 1)
    indptr, indices, groups = [0], [], {}
    for name, cols in _touched_sets(n).items():
        first = len(indptr) - 1
        at = 0
        while at < len(cols):
            m = int(min(rng.integers(1, 4), len(cols) - at))
            indices.extend(cols[at: at + m])
            indptr.append(len(indices))
            at += m
        groups[name] = np.arange(first, len(indptr) - 1, dtype=np.int32)
    n_rows = len(indptr) - 1
    X = csr_matrix((rng.standard_normal(len(indices)), np.array(indices, dtype=np.int32),
                    np.array(indptr, dtype=np.int64)), shape=(n_rows, n))
    log = {"features": X, "labels": (rng.random(n_rows) < 0.5).astype(np.int64),
           "pscores": rng.uniform(0.1, 1.0, size=n_rows) ** 0.5}
    return log, groups


def _ranges(n, variant):
    """64 ascending first columns inside 0..n-1.  0: what n_features * r / n_ranks gives (repeated
    starts when there are more ranks than columns); 1: starts on and beside a chunk edge, at 0 and at
    n - 1, some of them twice."""
    if variant == 0:
        return np.array([n * r // 64 for r in range(64)], dtype=np.int32)
    special = [c for c in (0, 0, CHUNK - 1, CHUNK, CHUNK, CHUNK + 1, n - 1, n - 1) if 0 <= c < n]
    rest = 64 - len(special)
    lo = np.sort(np.array(special + [n * r // rest for r in range(rest)], dtype=np.int32))
    assert len(lo) == 64 and lo[0] >= 0 and lo[-1] <= n - 1
    return lo


@pytest.mark.parametrize("n", [1, 63, 2048, 2049, 3 * 2048, 2048 * 257 + 3])
def test_record_list_edges(rt, n):
    """Consecutive calls on one plan, each on the rows of one group (so every list must be free of
    the lists before it: 'evens' then 'odds' are disjoint and interleaved), with 64 owner ranges
    and, for two of the sets, every capacity around the count."""
    k = 2
    log, groups = _list_log(n)
    sets = _touched_sets(n)
    n_rows = log["features"].shape[0]
    assert n_rows <= 6000
    dev = gf.DeviceLog(rt, log, k, n_rows, -1)  # no hot class: a list names the touched columns only
    params = gf.Params(rt, *gf.perturbed_init(n % 1000, n, k))
    try:
        for call, (name, ids) in enumerate(groups.items()):
            want = sets[name]
            np.testing.assert_array_equal(np.unique(log["features"][ids].indices), want)
            count = len(want)
            lo = _ranges(n, call % 2)
            want_bounds = np.concatenate([np.searchsorted(want, lo), [count]])
            g, _ = gf.dense_grad(dev, ids, params)
            G_V, g_w, g_w0 = gf.split_grad(g, n, k)
            caps = {count + 5}
            if name in ("ends", "full_chunk"):
                caps |= {0, 1, max(count - 1, 0), count}
            for cap in sorted(caps):
                rec = gf.grad_rows(dev, ids, params, cap, lo)
                assert rec.count == count, (name, cap, rec.count)  # the true count, whatever the room
                np.testing.assert_array_equal(rec.bounds, want_bounds, err_msg=f"{name} cap={cap}")
                r = rec.filled()
                assert len(r) == min(count, cap)
                np.testing.assert_array_equal(r[:, 0], want[: len(r)].astype(np.float64), err_msg=name)
                np.testing.assert_array_equal(r[:, 1: k + 1], G_V[want[: len(r)]])
                np.testing.assert_array_equal(r[:, k + 1], g_w[want[: len(r)]])
                assert rec.gw0 == g_w0
                rec.assert_rest_untouched()
    finally:
        dev.close()


# --------------------------------------------------------------------------
# E. the owner side (rfm_fm_reduce_rows), the stores (rfm_fm_set_rows), rfm_fm_apply_rows
# --------------------------------------------------------------------------
def _segments(rng, n, k, seg_cols):
    """Record lists back to back, one per entry of seg_cols (ascending columns each)."""
    segs = [np.concatenate([np.asarray(c, dtype=np.float64)[:, None], rng.standard_normal((len(c), k + 1))], axis=1)
            for c in seg_cols]
    rows = np.concatenate(segs) if segs else np.zeros((0, k + 2))
    seg_ptr = np.concatenate([[0], np.cumsum([len(c) for c in seg_cols])]).astype(np.int32)
    return rows, seg_ptr


def _reduce_oracle(rows, V, w, lr):
    """Sums in segment (= position) order, in float64; [column, V - lr * sum, w - lr * sum] at the
    column's first record, column -1 at its others.  Also the magnitude |theta| + |lr * sum|."""
    k = V.shape[1]
    want = np.full_like(rows, np.nan)
    want[:, 0] = -1.0
    mag = np.zeros_like(rows)
    acc, first = {}, {}
    for i, r in enumerate(rows):
        c = int(r[0])
        if c in first:
            acc[c] = acc[c] + r[1:]
        else:
            first[c], acc[c] = i, 0.0 + r[1:]
    for c, i in first.items():
        theta = np.concatenate([V[c], [w[c]]])
        want[i, 0] = c
        want[i, 1:] = theta - lr * acc[c]
        mag[i, 1:] = np.abs(theta) + np.abs(lr * acc[c])
    return want, mag


def _reduce_layouts(rng, n, n_seg):
    """Column lists per segment: a column in every segment and one in the last only; then the same
    with the first and the last segment empty (n_seg > 1)."""
    def draw():
        return np.sort(rng.choice(np.arange(8, n - 8), size=int(rng.integers(3, 14)), replace=False))
    full = [np.union1d(draw(), [5]) for _ in range(n_seg)]
    full[-1] = np.union1d(full[-1], [n - 1])  # column n - 1: the last segment only
    layouts = [full]
    if n_seg > 1:
        layouts.append([np.array([], dtype=np.int64)] + [draw() for _ in range(n_seg - 2)] + [np.array([], dtype=np.int64)])
        layouts.append([draw()] + [np.array([], dtype=np.int64)] * (n_seg - 1))
    return layouts


def _run_reduce(rt, rows, seg_ptr, V, w, lr):
    import torch
    from relevance_factorizationmachine_amd import _lib
    n, k = V.shape
    dV, dw = rt.upload(V), rt.upload(w)
    d_rows, d_seg = rt.upload(rows), rt.upload(seg_ptr)
    out = torch.full((len(rows) + gf.GUARD, k + 2), float("nan"), dtype=torch.float64, device=rt.torch_device)
    _lib.check(rt.lib.rfm_fm_reduce_rows(rt.ctx, d_rows.data_ptr(), d_seg.data_ptr(), len(seg_ptr) - 1, len(rows),
                                         dw.data_ptr(), dV.data_ptr(), n, k, lr, out.data_ptr()))
    rt.sync()
    np.testing.assert_array_equal(dV.cpu().numpy(), V)  # the owner's tables are read only
    return out


def _check_reduce_and_set(rt, rows, seg_ptr, V, w, lr, rng):
    from relevance_factorizationmachine_amd import _lib
    n, k = V.shape
    want, mag = _reduce_oracle(rows, V, w, lr)
    out = _run_reduce(rt, rows, seg_ptr, V, w, lr)
    res = out.cpu().numpy()
    assert np.isnan(res[len(rows):]).all()
    res = res[: len(rows)]
    np.testing.assert_array_equal(res[:, 0], want[:, 0])  # column fields and the -1 positions: exact
    live = want[:, 0] >= 0
    # the same numbers in the same order, except where the device fuses V - lr * sum: one rounding
    assert (np.abs(res[live, 1:] - want[live, 1:]) <= 2.0 ** -52 * mag[live, 1:]).all()
    # rfm_fm_set_rows into a replica with other contents
    V2, w2, w0 = rng.standard_normal((n, k)), rng.standard_normal(n), rng.standard_normal(1)
    dV2, dw2, dw0 = rt.upload(V2), rt.upload(w2), rt.upload(w0)
    parts = np.array([0.5, 1e300, -1.25, 1e300, 3.0, 1e300])
    d_parts = rt.upload(parts)
    _lib.check(rt.lib.rfm_fm_set_rows(rt.ctx, out.data_ptr(), len(rows), d_parts.data_ptr(), 3, 2,
                                      dw0.data_ptr(), dw2.data_ptr(), dV2.data_ptr(), n, k, lr))
    rt.sync()
    gV, gw, gw0 = dV2.cpu().numpy(), dw2.cpu().numpy(), dw0.cpu().numpy()
    cols = want[live, 0].astype(np.int64)
    np.testing.assert_array_equal(gV[cols], res[live, 1: k + 1])  # stored rows: the records' bits
    np.testing.assert_array_equal(gw[cols], res[live, k + 1])
    rest = np.setdiff1d(np.arange(n), cols)
    np.testing.assert_array_equal(gV[rest], V2[rest])  # the others (and the -1 records): untouched
    np.testing.assert_array_equal(gw[rest], w2[rest])
    s = (0.5 + -1.25) + 3.0
    assert abs(gw0[0] - (w0[0] - lr * s)) <= 2.0 ** -52 * (abs(w0[0]) + abs(lr * s))


@pytest.mark.parametrize("n_seg", [1, 2, 64])
@pytest.mark.parametrize("k", [1, 62, 63, 64, 65, 128, 400])
def test_reduce_rows_and_set_rows(rt, k, n_seg):
    """k + 1 values per record in trips of 64: the g_w slot is in the first trip up to k = 63, alone
    in the second at k = 64, and later beyond; 64 segments are the limit of the kernel's masks."""
    rng = np.random.default_rng(1000 * k + n_seg)
    n, lr = 300, 0.37
    V, w = rng.standard_normal((n, k)), rng.standard_normal(n)
    for seg_cols in _reduce_layouts(rng, n, n_seg):
        rows, seg_ptr = _segments(rng, n, k, seg_cols)
        _check_reduce_and_set(rt, rows, seg_ptr, V, w, lr, rng)


def test_reduce_rows_strides_over_the_records(rt):
    """12 000 records at k = 4: the launch is capped at 8 workgroups per CU of 4 waves each, one
    wave per record (8 192 records in flight on 256 CUs), so the record loop takes a second trip."""
    rng = np.random.default_rng(12)
    n, k, lr = 6000, 4, 0.37
    V, w = rng.standard_normal((n, k)), rng.standard_normal(n)
    seg_cols = [np.sort(rng.choice(n, size=4000, replace=False)) for _ in range(3)]
    rows, seg_ptr = _segments(rng, n, k, seg_cols)
    assert len(rows) == 12_000
    _check_reduce_and_set(rt, rows, seg_ptr, V, w, lr, rng)


@pytest.mark.parametrize("k", [65, 400])
def test_apply_rows_respects_capacity_and_null_gw0(rt, k):
    import torch
    from relevance_factorizationmachine_amd import _lib
    rng = np.random.default_rng(k)
    n, lr, cap = 500, 0.37, 40
    cols = np.sort(rng.choice(n, size=cap + 5, replace=False))
    rows, _ = _segments(rng, n, k, [cols])
    V, w, w0 = rng.standard_normal((n, k)), rng.standard_normal(n), rng.standard_normal(1)
    params = gf.Params(rt, w0, w, V)
    d_rows = rt.upload(rows)
    d_n = rt.upload(np.array([cap + 5], dtype=np.int32))  # a device count above cap_rows
    _lib.check(rt.lib.rfm_fm_apply_rows(rt.ctx, d_rows.data_ptr(), d_n.data_ptr(), cap, None, *params.ptrs(),
                                        n, k, lr))
    g0, gw, gV = params.host()
    assert g0[0] == w0[0]  # d_gw0 = NULL: w0 is left alone
    on, off = cols[:cap], np.setdiff1d(np.arange(n), cols[:cap])
    np.testing.assert_array_equal(gV[off], V[off])  # (the five records past cap_rows among them)
    np.testing.assert_array_equal(gw[off], w[off])
    step_V, step_w = lr * rows[:cap, 1: k + 1], lr * rows[:cap, k + 1]
    assert (np.abs(gV[on] - (V[on] - step_V)) <= 2.0 ** -52 * (np.abs(V[on]) + np.abs(step_V))).all()
    assert (np.abs(gw[on] - (w[on] - step_w)) <= 2.0 ** -52 * (np.abs(w[on]) + np.abs(step_w))).all()
    assert not np.array_equal(gV[on], V[on])
    # ... and with g_w0 given
    d_gw0 = rt.upload(np.array([1.5]))
    _lib.check(rt.lib.rfm_fm_apply_rows(rt.ctx, d_rows.data_ptr(), d_n.data_ptr(), 0, d_gw0.data_ptr(),
                                        *params.ptrs(), n, k, lr))
    h0, hw, hV = params.host()
    assert abs(h0[0] - (w0[0] - lr * 1.5)) <= 2.0 ** -52 * (abs(w0[0]) + lr * 1.5)
    np.testing.assert_array_equal(hV, gV)  # cap_rows = 0: no record applied
