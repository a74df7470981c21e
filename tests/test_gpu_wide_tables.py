"""Row addressing of the kernels in tables past 4 GiB (T32b) and past 2^31 elements (T31e).  Needs an
MI355X: ``pytest -m gpu``.

The method, the three assertions of every case -- (a) live rows against the compact run, (b) the
census of every wide table, (c) the sizes the case means -- and the id maps are
wide_tables_common.py's; test_wide_tables_host.py shows on a NumPy model that a wrapped offset fails
(a) or (b) on every map used here.  Each case prints the size of its wide table and the threshold
it crosses.  A case's factor count is the largest that takes the addressing path it means, so its
table has the fewest rows that cross the threshold.

Rows that a kernel reads although no example names them: the sequential MF kernel loads row 0 of P
and of Q into a slot that has no example yet (mf_ring_fetch: ``got_user ? e.u : 0``) and lanes past
the factor count reload a row's first factors (mf_load_row, load_v_row: ``f < k ? f : 0``).  Row 0
is a live id of every map, and the reloaded factors belong to the row that is read anyway, so the
census needs no allowance for either.

Peak device memory of a case is given in its docstring; every case asserts that much room first."""
import functools

import numpy as np
import pytest

import adagrad_common as ac
import forward_rows_common as fr
import grad_forms_common as gf
import mf_adagrad_common as ma
import mf_step_common as ms
import pair_tile_common as pt
import sliced_rows_common as sr
import wide_tables_common as wt

pytestmark = pytest.mark.gpu

GIB = wt.GIB
K_SHORT_SPLIT = 8   # kShortSplit of rfm_fm_kernels.hpp (as test_gpu_grad_forms.py)
STEP_LR = 2.0 ** -3


_release = wt.free_tables


@pytest.fixture(scope="module")
def rt():
    """The runtime; its finaliser frees whatever wide table the module still holds."""
    from relevance_factorizationmachine_amd import runtime
    yield runtime.Runtime.get()
    wt.free_tables()


@pytest.fixture(autouse=True)
def _free_tables():
    """Every wide table is registered where it is made (wide_tables_common.nan_table) and its
    storage emptied here, after the case -- also one that a failed case's traceback still holds, so
    a failure cannot leave the next case short of room."""
    yield
    wt.free_tables()


def _announce(imap, what):
    print("\n" + imap.describe(what))


# --------------------------------------------------------------------------
# FM
# --------------------------------------------------------------------------
def _lpr(k):
    return gf.CLASS_OF[k][0]


@functools.lru_cache(maxsize=None)
def _fm_case(map_name, k, n_rows, bounded=False):
    """A compact log of the map's columns with one column in (almost) every row, moved to the
    compact id whose wide id is the table's highest threshold row T; parameters scaled so that the
    scores do not saturate (forward_rows_common.forward_params); the full batch in shuffled order;
    the wide twin of the log."""
    imap = wt.id_map(map_name)
    assert imap.width == k
    rng = np.random.default_rng(31 * k + n_rows)
    if bounded:   # rows of at most 16 entries: the plan keeps padded row blocks
        log = gf._bounded_log(rng, n_rows, imap.m, 16, 1)
    else:
        log = gf.split_case(k, n_rows, imap.m, 1, 1000 + 7 * k + n_rows)[0]
    theta = fr.forward_params(2000 + k, imap.m, k, _lpr(k))
    log, theta = wt.move_column(log, theta, 0, imap.compact(imap.top))
    # (every row that has an entry at all: a bounded log draws a seventeenth of its rows empty)
    assert log["features"].getnnz(axis=0)[imap.compact(imap.top)] == (np.diff(log["features"].indptr) > 0).sum()
    full = rng.permutation(n_rows).astype(np.int32)
    return imap, log, theta, full, wt.widen_log(log, imap)


def _wide_params(rt, imap, theta, what):
    wt.assert_room(rt, imap.n * (imap.width + 1) * 8)
    p = wt.WideFmParams(rt, imap, *theta)
    p.assert_sizes()
    p.assert_census(f"{what} before the call")
    _announce(imap, what)
    return p


def _assert_hot_state(dev, imap, hot, n_rows, k):
    """The column at T went the way the case means: a hot column (modes 0 and -2 at a single-chunk
    factor count), else a split column once the rows outnumber a workgroup's slots."""
    info = dev.plan.info()
    assert dev.plan.layout()["lanes_per_row"] == _lpr(k)
    if hot != -1 and not gf.chunked(k):
        assert imap.top in dev.plan.hot_columns().tolist(), (info, dev.plan.hot_columns())
        return "hot"
    assert info["hot_columns"] == 0 and info["split_columns"] >= 1, info
    return "split"


FORWARD_KS = (32, 128, 1024)   # 16 lanes, 64 lanes in one chunk, 64 lanes in 8 chunks


@pytest.mark.parametrize("k", FORWARD_KS)
def test_fm_forward_csr(rt, k):
    """rfm_fm_forward through the caller's CSR, one row per lane group.  Peak: V 4 GiB."""
    imap, log, theta, _, wlog = _fm_case(f"fm-V-k{k}", k, 293)
    n_rows = log["features"].shape[0]
    assert fr.forward_geometry(rt, n_rows, k, False)["block"] == 256
    want = fr.forward(rt, fr.DeviceRows(rt, log), gf.Params(rt, *theta), n_rows)
    params = _wide_params(rt, imap, theta, f"rfm_fm_forward k={k}")
    got = fr.forward(rt, fr.DeviceRows(rt, wlog), params, n_rows)
    assert np.isfinite(want).all() and fr.unsaturated_share(fr.row_oracle(log["features"], *theta)) > 0.8
    wt.assert_same_bits(got, want, "scores")
    params.assert_census("after rfm_fm_forward")


def test_fm_forward_csr_many_rows_shape(rt):
    """rfm_fm_forward at the smallest row count of the 1 024-thread shape (several rows in flight per
    lane group: the second gather of rfm_fm_kernels.hpp).  Peak: V 4 GiB."""
    k = 128
    n_rows = fr.many_rows_minimum(rt, k, False) + 1
    assert n_rows <= gf.GRAD_TOL_ROWS
    imap, log, theta, _, wlog = _fm_case(f"fm-V-k{k}", k, n_rows)
    assert fr.forward_geometry(rt, n_rows, k, False)["block"] == 1024
    want = fr.forward(rt, fr.DeviceRows(rt, log), gf.Params(rt, *theta), n_rows)
    params = _wide_params(rt, imap, theta, f"rfm_fm_forward, many-rows shape, k={k}, {n_rows} rows")
    got = fr.forward(rt, fr.DeviceRows(rt, wlog), params, n_rows)
    assert np.isfinite(want).all()
    wt.assert_same_bits(got, want, "scores")
    params.assert_census("after rfm_fm_forward")


@pytest.mark.parametrize("k,sliced", [(128, False), (1024, False), (1024, True)],
                         ids=["plain-k128", "plain-k1024", "sliced-k1024"])
def test_fm_plan_forward(rt, monkeypatch, k, sliced):
    """rfm_fm_plan_forward in the plain form (16 to 64 lanes per row) and in the form sliced by
    factors, whose workgroups copy the frequent columns' slices of V into LDS.  Peak: V 4 GiB."""
    monkeypatch.setenv("RFM_SLICED_MIN_ROWS", "1" if sliced else str(1 << 30))
    imap, log, theta, _, wlog = _fm_case(f"fm-V-k{k}", k, 293)
    n_rows = log["features"].shape[0]
    outs = []
    for lg, make in ((log, lambda: gf.Params(rt, *theta)),
                     (wlog, lambda: _wide_params(rt, imap, theta, f"rfm_fm_plan_forward k={k} sliced={sliced}"))):
        dev = gf.DeviceLog(rt, lg, k, 64)
        try:
            assert (dev.plan.sliced()["slices"] > 0) == (k > 128)
            assert dev.plan.sliced_geometry(n_rows)["sliced"] == int(sliced)
            if sliced and lg is wlog:   # the column at T is one of those a workgroup keeps in LDS
                assert imap.top in dev.plan.sliced_columns().tolist()
            params = make()
            outs.append(sr.plan_forward(rt, dev.plan, fr.DeviceRows(rt, lg), params, n_rows))
        finally:
            dev.close()
    assert np.isfinite(outs[0]).all()
    wt.assert_same_bits(outs[1], outs[0], "scores")
    params.assert_census("after rfm_fm_plan_forward")


# (factor count, hot mode, split form of the column at T where it is a split column, rule)
STEP_CASES = [
    (128, -1, "short", "sgd"), (128, -1, "long", "sgd"), (128, 0, "short", "sgd"), (128, -2, "short", "sgd"),
    (1024, 0, "short", "sgd"), (1024, 0, "long", "sgd"),
    (128, -1, "short", "adagrad"), (128, -2, "short", "adagrad"), (128, 0, "short", "adagrad"),
    (1024, 0, "short", "adagrad"),
]


def _step_rows(k, form):
    bc = gf.full_batch_workgroup_slots(k)
    return (bc if form == "short" else K_SHORT_SPLIT * bc) + 37


@functools.lru_cache(maxsize=None)
def _step_oracle(map_name, k, n_rows, bounded=False):
    imap, log, theta, full, _ = _fm_case(map_name, k, n_rows, bounded)
    return gf.grad_oracle(log, full, *theta)


@pytest.mark.parametrize("k,hot,form,rule", STEP_CASES,
                         ids=[f"k{k}-hot{hot}-{form}-{rule}" for k, hot, form, rule in STEP_CASES])
def test_fm_step(rt, k, hot, form, rule):
    """One rfm_fm_step on the full batch under SGD or AdaGrad (wide acc_V and acc_w beside V and w).
    The column at T is in every row: a hot column under modes 0 and -2 (consume_hot_column), a split
    column under -1 and at chunked factor counts (short finalize: up to 8 partial rows, long: more).
    Peak: V 4 GiB, AdaGrad 8 GiB."""
    map_name = f"fm-V-k{k}"
    n_rows = _step_rows(k, form)
    imap, log, theta, full, wlog = _fm_case(map_name, k, n_rows)
    fixed = gf.fixed_order(k, hot)
    acc0 = ac.acc_init("uniform", imap.m, k, k) if rule == "adagrad" else None
    results = []
    for lg in (log, wlog):
        dev = gf.DeviceLog(rt, lg, k, n_rows, hot)
        try:
            if lg is wlog:
                state = _assert_hot_state(dev, imap, hot, n_rows, k)
                if state == "split":
                    parts = -(-int(log["features"].getnnz(axis=0)[imap.compact(imap.top)]) // dev.geometry()["BC"])
                    assert (2 <= parts <= K_SHORT_SPLIT) if form == "short" else parts > K_SHORT_SPLIT, parts
                params = _wide_params(rt, imap, theta, f"rfm_fm_step k={k} hot={hot} {form} {rule}: V")
                accs = _wide_params(rt, imap, acc0, "acc_V") if acc0 is not None else None
            else:
                params = gf.Params(rt, *theta)
                accs = gf.Params(rt, *acc0) if acc0 is not None else None
            if rule == "adagrad":
                ac.adagrad_step(dev, full, params, accs, STEP_LR)
            else:
                gf.step(dev, full, params, STEP_LR)
            if lg is wlog:
                params.assert_census("after rfm_fm_step")
                results.append((params.live(), accs.live() if accs is not None else None))
                if accs is not None:
                    accs.assert_census("accumulators after rfm_fm_step")
            else:
                results.append((params.host(), accs.host() if accs is not None else None))
        finally:
            dev.close()
    (c_theta, c_acc), (w_theta, w_acc) = results
    at = imap.compact(imap.top)
    assert not np.array_equal(c_theta[2][at], theta[2][at])   # the column at T moved
    if fixed:
        for name, a, b in zip(("w0", "w", "V"), w_theta, c_theta):
            wt.assert_same_bits(a, b, name)
        if w_acc is not None:
            for name, a, b in zip(("acc_w0", "acc_w", "acc_V"), w_acc, c_acc):
                wt.assert_same_bits(a, b, name)
    else:   # arrival-order hot sums: the bound of the call's own module against the compact oracle
        oracle = _step_oracle(map_name, k, n_rows)
        for got_theta, got_acc in ((c_theta, c_acc), (w_theta, w_acc)):
            if rule == "adagrad":
                ac.assert_inside(got_theta, got_acc, theta, acc0, oracle, STEP_LR, ac.EPS, n_rows, f"k={k} hot={hot}")
            else:
                for name, ratio in zip(("w0", "w", "V"), gf.step_excess(got_theta, theta, oracle, STEP_LR, n_rows)):
                    print(f"{name}: worst |got - (theta - lr g)| / bound = {float(ratio.max()):.3g}")
                    assert (ratio <= 1).all(), (name, np.argwhere(ratio > 1)[:5], float(ratio.max()))


def test_fm_step_8_lane_forward(rt):
    """The step's forward at 8 lanes per row (k = 32, padded row blocks, many-rows shape, arrival-order
    hot sums: the column at T is the one hot column), then the gradient launch.  16.8 M columns.
    Peak: V 4 GiB, w 0.13 GiB."""
    k, map_name = 32, "fm-V-k32-bounded"
    n_rows = fr.many_rows_minimum(rt, k, True)
    assert n_rows <= gf.GRAD_TOL_ROWS
    imap, log, theta, full, wlog = _fm_case(map_name, k, n_rows, True)
    oracle = _step_oracle(map_name, k, n_rows, True)
    for lg in (log, wlog):
        dev = gf.DeviceLog(rt, lg, k, n_rows, n_rows // 2)   # hot: a column in half the rows of a batch
        try:
            form = dev.plan.step_form(n_rows)
            assert dev.plan.layout()["row_blocks"] == 1 and form["lanes8"] == 1 and form["lanes"] == 8, form
            assert form["kind"] == "blocks" and not form["fixed_order"], form
            hot_cols = dev.plan.hot_columns().tolist()
            assert hot_cols == [imap.top if lg is wlog else imap.compact(imap.top)], hot_cols
            params = _wide_params(rt, imap, theta, f"rfm_fm_step, 8-lane forward, {n_rows} rows") if lg is wlog \
                else gf.Params(rt, *theta)
            gf.step(dev, full, params, STEP_LR)
            if lg is wlog:
                params.assert_census("after rfm_fm_step")
            got = params.live() if lg is wlog else params.host()
            for name, ratio in zip(("w0", "w", "V"), gf.step_excess(got, theta, oracle, STEP_LR, n_rows)):
                print(f"{'wide' if lg is wlog else 'compact'} {name}: worst / bound = {float(ratio.max()):.3g}")
                assert (ratio <= 1).all(), (name, np.argwhere(ratio > 1)[:5], float(ratio.max()))
        finally:
            dev.close()


def _wide_dense_grad(rt, dev, ids, params):
    """rfm_fm_grad into a NaN-filled device buffer of n (k + 1) + 1 doubles (it stays on the device)."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    d_ids = rt.upload(np.asarray(ids, dtype=np.int32))
    grad = wt.nan_table(rt, (dev.n * (dev.k + 1) + 1,))
    _lib.check(rt.lib.rfm_fm_grad(rt.ctx, dev.plan.handle, *dev.log_ptrs(), d_ids.data_ptr(), len(ids),
                                  *params.ptrs(), grad.data_ptr()))
    rt.sync()
    return grad


@pytest.mark.parametrize("k,hot", [(128, -1), (128, 0), (128, -2), (1024, 0)])
def test_fm_grad_dense(rt, k, hot):
    """rfm_fm_grad into a wide dense gradient [G_V (n k) | g_w (n) | g_w0]: with n k past 2^29 the
    whole g_w region and g_w0 lie past 4 GiB.  Every element is written (the census is the whole
    buffer), the non-zero elements are as many as the compact gradient's.  Peak: V and the gradient,
    8 GiB."""
    map_name = f"fm-V-k{k}"
    n_rows = _step_rows(k, "short")
    imap, log, theta, full, wlog = _fm_case(map_name, k, n_rows)
    cdev = gf.DeviceLog(rt, log, k, n_rows, hot)
    try:
        g_c, _ = gf.dense_grad(cdev, full, gf.Params(rt, *theta))
    finally:
        cdev.close()
    c_V, c_w, c_w0 = gf.split_grad(g_c, imap.m, k)
    dev = gf.DeviceLog(rt, wlog, k, n_rows, hot)
    try:
        _assert_hot_state(dev, imap, hot, n_rows, k)
        wt.assert_room(rt, 2 * imap.n * (k + 1) * 8)
        params = _wide_params(rt, imap, theta, f"rfm_fm_grad k={k} hot={hot}: V and a gradient of the same size")
        grad = _wide_dense_grad(rt, dev, full, params)
    finally:
        dev.close()
    n = imap.n
    assert grad.numel() * 8 > 2 ** 32 and (n * k + imap.wide[0]) * 8 >= 2 ** 32
    assert wt.census(grad) == grad.numel(), "an element of the wide gradient was not written"
    assert wt.count_nonzero(grad) == int(np.count_nonzero(g_c))
    w_V = wt.live_rows(grad[: n * k].view(n, k), imap.wide)
    w_w = wt.live_rows(grad[n * k: n * k + n], imap.wide)
    w_w0 = float(grad[n * k + n].cpu())
    if gf.fixed_order(k, hot):
        wt.assert_same_bits(w_V, c_V, "G_V")
        wt.assert_same_bits(w_w, c_w, "g_w")
        wt.assert_same_bits(w_w0, c_w0, "g_w0")
    else:
        o_w0, o_w, o_V, (S_0, S_w, S_V) = _step_oracle(map_name, k, n_rows)
        tol = gf.grad_tol(n_rows)
        gf.assert_within_scale(w_V, o_V, S_V, tol, "G_V")
        gf.assert_within_scale(w_w, o_w, S_w, tol, "g_w")
        gf.assert_within_scale(w_w0, o_w0, S_0, tol, "g_w0")
    params.assert_census("after rfm_fm_grad")


def _reduce_and_set(rt, rec, params, n, k, lr):
    """rfm_fm_reduce_rows on the list of `rec` as two segments (the same list twice: every column's
    records are added in segment order), then rfm_fm_set_rows of the result into `params`; the
    reduced records on the host."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    cnt = rec.count
    both = torch.cat([rec.d_rows[:cnt], rec.d_rows[:cnt]]).contiguous()
    seg = rt.upload(np.array([0, cnt, 2 * cnt], dtype=np.int32))
    out = torch.full((2 * cnt + gf.GUARD, k + 2), float("nan"), dtype=torch.float64, device=rt.torch_device)
    w0, w, V = params.ptrs()
    _lib.check(rt.lib.rfm_fm_reduce_rows(rt.ctx, both.data_ptr(), seg.data_ptr(), 2, 2 * cnt, w, V, n, k, lr,
                                         out.data_ptr()))
    _lib.check(rt.lib.rfm_fm_set_rows(rt.ctx, out.data_ptr(), 2 * cnt, rec.d_gw0.data_ptr(), 1, 1, w0, w, V, n, k, lr))
    rt.sync()
    got = out.cpu().numpy()
    assert np.isnan(got[2 * cnt:]).all()
    return got[: 2 * cnt]


@pytest.mark.parametrize("k,hot", [(128, -2), (128, -1), (1024, 0)])
def test_fm_record_lists(rt, k, hot):
    """rfm_fm_grad_rows (records ascending by wide column, owner ranges that start on either side of
    T), rfm_fm_apply_rows into a wide V, then rfm_fm_reduce_rows and rfm_fm_set_rows with record
    columns past T.  Fixed-order modes: the records are the compact run's, the column under the map.
    Peak: two V, 8 GiB."""
    map_name = f"fm-V-k{k}"
    n_rows = _step_rows(k, "short")
    imap, log, theta, full, wlog = _fm_case(map_name, k, n_rows)
    assert gf.fixed_order(k, hot)
    T = imap.top
    w_ranges = [0, 3, T - 1, T, T + 1, imap.n - 1]
    c_ranges = [0, 3] + [imap.compact(c) for c in w_ranges[2:]]
    from relevance_factorizationmachine_amd import _lib
    out = []
    for lg, ranges in ((log, c_ranges), (wlog, w_ranges)):
        dev = gf.DeviceLog(rt, lg, k, n_rows, hot)
        try:
            wide = lg is wlog
            n = imap.n if wide else imap.m
            make = (lambda what: _wide_params(rt, imap, theta, what)) if wide else (lambda what: gf.Params(rt, *theta))
            params = make(f"rfm_fm_grad_rows / rfm_fm_apply_rows k={k} hot={hot}")
            rec = gf.grad_rows(dev, full, params, imap.m, ranges)
            rec.assert_rest_untouched()
            _lib.check(rt.lib.rfm_fm_apply_rows(rt.ctx, rec.d_rows.data_ptr(), rec.d_n.data_ptr(), imap.m,
                                                rec.d_gw0.data_ptr(), *params.ptrs(), n, k, STEP_LR))
            rt.sync()
            applied = params.live() if wide else params.host()
            other = make(f"rfm_fm_reduce_rows / rfm_fm_set_rows k={k}")
            reduced = _reduce_and_set(rt, rec, other, n, k, STEP_LR)
            if wide:
                params.assert_census("after rfm_fm_apply_rows")
                other.assert_census("after rfm_fm_set_rows")
            out.append((rec, applied, reduced, other.live() if wide else other.host()))
        finally:
            dev.close()
    (c_rec, c_applied, c_red, c_set), (w_rec, w_applied, w_red, w_set) = out
    assert w_rec.count == c_rec.count > 4
    cols = w_rec.filled()[:, 0].astype(np.int64)
    np.testing.assert_array_equal(cols, imap(c_rec.filled()[:, 0].astype(np.int64)))
    assert {T - 1, T, T + 1, imap.n - 1} <= set(cols.tolist())   # record columns on either side of T
    wt.assert_same_bits(w_rec.filled()[:, 1:], c_rec.filled()[:, 1:], "records")
    assert w_rec.gw0 == c_rec.gw0
    np.testing.assert_array_equal(w_rec.bounds, c_rec.bounds)
    assert len(set(w_rec.bounds[2:5].tolist())) == 3   # T - 1, T and T + 1 start lists of their own
    for name, a, b in zip(("w0", "w", "V"), w_applied, c_applied):
        wt.assert_same_bits(a, b, f"{name} after rfm_fm_apply_rows")
    first = c_red[:, 0] >= 0
    np.testing.assert_array_equal(w_red[:, 0] >= 0, first)
    np.testing.assert_array_equal(w_red[first, 0].astype(np.int64), imap(c_red[first, 0].astype(np.int64)))
    np.testing.assert_array_equal(w_red[~first, 0], c_red[~first, 0])
    wt.assert_same_bits(w_red[first, 1:], c_red[first, 1:], "reduced records")
    for name, a, b in zip(("w0", "w", "V"), w_set, c_set):
        wt.assert_same_bits(a, b, f"{name} after rfm_fm_set_rows")
    assert not np.array_equal(c_set[2], theta[2])


def test_fm_forward_and_step_past_2_31_elements(rt):
    """T31e for the FM family at its largest factor count, 1 024: V of 2.1 M columns is just over
    16 GiB and crosses both thresholds; rfm_fm_forward, then one SGD step on the full batch (the
    column at the T31e row is a split column of the short finalize).  No gradient table.
    Peak: V 16 GiB."""
    k, map_name = 1024, "fm-V-k1024-T31e"
    n_rows = _step_rows(k, "short")
    imap, log, theta, full, wlog = _fm_case(map_name, k, n_rows)
    assert set(imap.kinds) == {wt.T32B, wt.T31E} and imap.top == imap.T[wt.T31E]
    want = fr.forward(rt, fr.DeviceRows(rt, log), gf.Params(rt, *theta), n_rows)
    cdev = gf.DeviceLog(rt, log, k, n_rows, 0)
    try:
        cparams = gf.Params(rt, *theta)
        gf.step(cdev, full, cparams, STEP_LR)
        c_theta = cparams.host()
    finally:
        cdev.close()
    params = _wide_params(rt, imap, theta, "rfm_fm_forward and rfm_fm_step, k=1024")
    assert params.V.numel() > 2 ** 31
    got = fr.forward(rt, fr.DeviceRows(rt, wlog), params, n_rows)
    wt.assert_same_bits(got, want, "scores")
    dev = gf.DeviceLog(rt, wlog, k, n_rows, 0)
    try:
        assert _assert_hot_state(dev, imap, 0, n_rows, k) == "split"
        gf.step(dev, full, params, STEP_LR)
    finally:
        dev.close()
    params.assert_census("after rfm_fm_step")
    assert not np.array_equal(c_theta[2][imap.compact(imap.top)], theta[2][imap.compact(imap.top)])
    for name, a, b in zip(("w0", "w", "V"), params.live(), c_theta):
        wt.assert_same_bits(a, b, name)


# --------------------------------------------------------------------------
# MF
# --------------------------------------------------------------------------
class WideMf:
    """P, Q, b_u, b_i (or their accumulators) on the device, the users' or the items' tables wide:
    `umap` / `imap` an IdMap, or None for a table of the compact size."""

    def __init__(self, rt, umap, imap, P, Q, bu, bi):
        self.rt = rt
        self.maps = (umap, imap, umap, imap)
        self.tables = []
        for m, a in zip(self.maps, (P, Q, bu, bi)):
            n, live = (m.n, m.wide) if m is not None else (len(a), np.arange(len(a)))
            self.tables.append(wt.wide_table(rt, n, a.shape[1] if a.ndim == 2 else None, live, a))

    def ptrs(self):
        return tuple(t.data_ptr() for t in self.tables)

    def host(self):
        """The four arrays at the live ids: the shapes of the compact problem."""
        self.rt.sync()
        return tuple(wt.live_rows(t, m.wide) if m is not None else t.cpu().numpy() for m, t in zip(self.maps, self.tables))

    def assert_census(self, what):
        self.rt.sync()
        for name, m, t in zip(("P", "Q", "b_u", "b_i"), self.maps, self.tables):
            wt.assert_census(t, m.m if m is not None else t.shape[0], f"{what} {name}")


def _mf_maps(side, make):
    """(user map, item map) of a case whose `side` table is wide."""
    return (make(), None) if side == "P" else (None, make())


def _wide_mf(rt, umap, imap, arrays, what):
    m = umap if umap is not None else imap
    wt.assert_room(rt, m.n * (m.width + 1) * 8)
    state = WideMf(rt, umap, imap, *arrays)
    m.assert_sizes(state.tables[0 if umap is not None else 1].numel())
    state.assert_census(f"{what} before the call")
    _announce(m, what)
    return state


def _assert_scored_ids_cross(prob, umap, imap):
    """The rows the call scores name wide ids below T, T itself and ids above it."""
    m = umap if umap is not None else imap
    ids = m(prob["users" if umap is not None else "items"][prob["sel"]])
    assert (ids < m.top).any() and (ids == m.top).any() and (ids > m.top).any(), np.unique(ids)


def _wide_predict(rt, prob, umap, imap, loss, what):
    """ms.run_predict on the wide twin of a predict_problem: (scores, loss or None)."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    users = umap(prob["users"]) if umap is not None else prob["users"]
    items = imap(prob["items"]) if imap is not None else prob["items"]
    state = _wide_mf(rt, umap, imap, prob["params"], what)
    n = prob["n_rows"]
    du, di = rt.upload(users.astype(np.int32)), rt.upload(items.astype(np.int32))
    d_ids = rt.upload(prob["ids"]) if prob["ids"] is not None else None
    ids_ptr = d_ids.data_ptr() if d_ids is not None else None
    out = torch.full((n + 8,), float("nan"), dtype=torch.float64, device=rt.torch_device)
    d_loss = torch.full((1,), float("nan"), dtype=torch.float64, device=rt.torch_device)
    if not loss:
        _lib.check(rt.lib.rfm_mf_predict(rt.ctx, du.data_ptr(), di.data_ptr(), ids_ptr, n, *state.ptrs(), ms.B0,
                                         prob["k"], out.data_ptr()))
    else:
        dy, dp = rt.upload(prob["y"]), rt.upload(prob["p"])
        _lib.check(rt.lib.rfm_mf_predict_loss(rt.ctx, du.data_ptr(), di.data_ptr(), dy.data_ptr(), dp.data_ptr(),
                                              ids_ptr, n, *state.ptrs(), ms.B0, prob["k"], ms.LOSS_EPS,
                                              out.data_ptr(), d_loss.data_ptr()))
    state.assert_census(f"after {what}")
    for a, b in zip(state.host(), prob["params"]):
        np.testing.assert_array_equal(a, b)
    got = out.cpu().numpy()
    assert np.isnan(got[n:]).all()
    return got[:n], (float(d_loss.cpu()[0]) if loss else None)


@pytest.mark.parametrize("with_ids", [False, True], ids=["rows-in-order", "row_ids"])
@pytest.mark.parametrize("loss", [False, True], ids=["predict", "predict_loss"])
@pytest.mark.parametrize("side", ["P", "Q"])
def test_mf_predict(rt, side, loss, with_ids):
    """rfm_mf_predict / rfm_mf_predict_loss at k = 128 with P (and b_u) or Q (and b_i) wide.
    Peak: 4 GiB."""
    k, n_rows = 128, 300
    prob = ms.predict_problem(k, n_rows, with_ids)
    assert ms.shape_class(k) == (64, 2, 1) and ms.CLASS_RANGE[(64, 2, 1)][1] == k
    umap, imap = _mf_maps(side, lambda: wt.id_map(f"mf-{side}-predict-k{k}"))
    _assert_scored_ids_cross(prob, umap, imap)
    want, want_loss = ms.run_predict(rt, prob, loss)
    got, got_loss = _wide_predict(rt, prob, umap, imap, loss, f"rfm_mf_predict{'_loss' if loss else ''}, {side} wide")
    wt.assert_same_bits(got, want, "scores")
    if loss:
        assert np.isfinite(want_loss)
        wt.assert_same_bits(got_loss, want_loss, "loss")


def _wide_schedule(case, umap, imap):
    """The case's batch under the maps and its schedule from the library's host scheduler: the
    compact schedule's records with the ids mapped."""
    from relevance_factorizationmachine_amd.runtime import mf_schedule_ex
    users = umap(case.users) if umap is not None else case.users
    items = imap(case.items) if imap is not None else case.items
    y, p = case.ry()
    cap = ms.capacity(case.k) if case.cache_cap is None else case.cache_cap
    n_users = umap.n if umap is not None else case.n_users
    n_items = imap.n if imap is not None else case.n_items
    sched = mf_schedule_ex(users, items, y, p, n_users, n_items, cap)
    ex, lptr, cache = ms.reach(case)
    np.testing.assert_array_equal(sched[1], lptr)
    np.testing.assert_array_equal(sched[0]["u"], umap(ex["u"]) if umap is not None else ex["u"])
    np.testing.assert_array_equal(sched[0]["i"], imap(ex["i"]) if imap is not None else ex["i"])
    for name in ("cslot", "gap", "ry"):
        np.testing.assert_array_equal(sched[0][name], ex[name])
    np.testing.assert_array_equal(sched[2], imap(cache) if imap is not None else cache)
    return sched, (ex, lptr, cache)


def _step_maps(name, case, side):
    return _mf_maps(side, lambda: wt.step_map(name, case.n_users if side == "P" else case.n_items))


@pytest.mark.parametrize("side", ["P", "Q"])
def test_mf_exact_step(rt, side):
    """rfm_mf_sgd_levels_ex on shape_case(128): a wide level (the grid kernel) in front of a
    sequential run of 24 levels on three cached items (the sequential kernel, its item cache and its
    read-ahead ring), the batch's users or items under the map.  Peak: 4 GiB."""
    name = "shape-k128"
    case = wt.mf_step_case(name)
    umap, imap = _step_maps(name, case, side)
    sched, compact = _wide_schedule(case, umap, imap)
    m = umap if umap is not None else imap
    ids = sched[0]["u" if side == "P" else "i"]
    assert (ids >= m.top).any() and (ids < m.top).any()
    if side == "Q":
        assert (sched[2] >= m.top).any(), "no cached item past T"
    init = case.init()
    want = ms.run_levels_ex(rt, case, compact, init)
    from relevance_factorizationmachine_amd import _lib
    ex, lptr, cache = sched
    state = _wide_mf(rt, umap, imap, init, f"rfm_mf_sgd_levels_ex, {side} wide")
    d_ex, d_lptr, d_cache = ma.upload_schedule(rt, sched)
    _lib.check(rt.lib.rfm_mf_sgd_levels_ex(
        rt.ctx, d_ex.data_ptr(), lptr.ctypes.data, d_lptr.data_ptr(), len(lptr) - 1,
        d_cache.data_ptr() if len(cache) else None, len(cache), *state.ptrs(), ms.B0, case.k, ms.LR, ms.REG))
    state.assert_census("after rfm_mf_sgd_levels_ex")
    for nm, a, b in zip(("P", "Q", "b_u", "b_i"), state.host(), want):
        wt.assert_same_bits(a, b, nm)
    assert not np.array_equal(want[0], init[0]) and not np.array_equal(want[1], init[1])


class _MfState:
    def __init__(self, params, accs):
        self.params, self.accs = params, accs


@pytest.mark.parametrize("side", ["P", "Q"])
def test_mf_adagrad_step(rt, side):
    """rfm_mf_sgd_levels_opt under AdaGrad on the same case: the parameters and their accumulators
    wide on the same side.  Peak: 8 GiB."""
    from optimizer_common import ADAGRAD
    from relevance_factorizationmachine_amd import _lib
    name = "shape-k128"
    case = wt.mf_step_case(name)
    umap, imap = _step_maps(name, case, side)
    sched, compact = _wide_schedule(case, umap, imap)
    init, acc0 = case.init(), ma.acc_init(case, "uniform")
    want = ma.run_levels_opt(rt, case, compact, init, acc0)
    state = _MfState(_wide_mf(rt, umap, imap, init, f"rfm_mf_sgd_levels_opt, {side} wide"),
                     _wide_mf(rt, umap, imap, acc0, f"rfm_mf_sgd_levels_opt, accumulators of {side} wide"))
    _lib.check(ma.call_opt(rt, case.k, sched, ma.upload_schedule(rt, sched), state, ADAGRAD))
    state.params.assert_census("after rfm_mf_sgd_levels_opt")
    state.accs.assert_census("accumulators after rfm_mf_sgd_levels_opt")
    for nm, a, b in zip(ma.NAMES, state.params.host() + state.accs.host(), want):
        wt.assert_same_bits(a, b, nm)
    assert not np.array_equal(want[4], acc0[0])


def test_mf_predict_and_step_past_2_31_elements(rt):
    """T31e for the MF family at its largest factor count, 1 024: P of 2.1 M users is just over 16 GiB;
    rfm_mf_predict, then rfm_mf_sgd_levels_ex on shape_case(1024).  Peak: 16 GiB."""
    k = 1024
    prob = ms.predict_problem(k, 300, True)
    umap = wt.id_map("mf-P-predict-k1024-T31e")
    assert umap.top == umap.T[wt.T31E]
    _assert_scored_ids_cross(prob, umap, None)
    want, _ = ms.run_predict(rt, prob, False)
    got, _ = _wide_predict(rt, prob, umap, None, False, "rfm_mf_predict k=1024, P wide")
    wt.assert_same_bits(got, want, "scores")
    _release()
    name = "shape-k1024-T31e"
    case = wt.mf_step_case(name)
    umap, imap = _step_maps(name, case, "P")
    sched, compact = _wide_schedule(case, umap, None)
    assert (sched[0]["u"] >= umap.T[wt.T31E]).any() and umap.n * k > 2 ** 31
    init = case.init()
    want = ms.run_levels_ex(rt, case, compact, init)
    from relevance_factorizationmachine_amd import _lib
    ex, lptr, cache = sched
    state = _wide_mf(rt, umap, None, init, "rfm_mf_sgd_levels_ex k=1024, P wide")
    d_ex, d_lptr, d_cache = ma.upload_schedule(rt, sched)
    _lib.check(rt.lib.rfm_mf_sgd_levels_ex(
        rt.ctx, d_ex.data_ptr(), lptr.ctypes.data, d_lptr.data_ptr(), len(lptr) - 1,
        d_cache.data_ptr() if len(cache) else None, len(cache), *state.ptrs(), ms.B0, case.k, ms.LR, ms.REG))
    state.assert_census("after rfm_mf_sgd_levels_ex")
    for nm, a, b in zip(("P", "Q", "b_u", "b_i"), state.host(), want):
        wt.assert_same_bits(a, b, nm)


# --------------------------------------------------------------------------
# pairs
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def rfm(rt):
    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import features, recommend
    return pkg, features, recommend, rt


def _wide_scores(rt, A, LU, Bw, LIw, c, n_items):
    """rfm_pair_scores of every user against a wide B that is on the device already -> the output
    [n_users, n_items] on the device, NaN-filled beforehand, a guard behind it."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    dA, dLU = rt.upload(pt._padded(A)), rt.upload(np.array(LU, dtype=np.float64))
    dc = rt.upload(np.array([c], dtype=np.float64))
    out = wt.nan_table(rt, (A.shape[0] * n_items + pt.GUARD,))
    _lib.check(rt.lib.rfm_pair_scores(rt.ctx, dA.data_ptr(), dLU.data_ptr(), A.shape[0], None, A.shape[0],
                                      Bw.data_ptr(), LIw.data_ptr(), n_items, A.shape[1], dc.data_ptr(), out.data_ptr()))
    rt.sync()
    assert bool(out[A.shape[0] * n_items:].isnan().all()), "an element past the output was written"
    return out[: A.shape[0] * n_items].view(A.shape[0], n_items)


@pytest.mark.parametrize("map_name", ["pair-B-kpad1024", "pair-B-kpad1024-T31e"])
def test_pair_scores_wide_b(rfm, map_name):
    """rfm_pair_scores against a wide B at the largest operand width, kpad = 1 024 (T32b: 0.5 M items,
    T31e: 2.1 M items).  The tile reads EVERY item's row, so the guard items score NaN: the live
    items' scores are the compact call's bit for bit (one logit per pair, a fixed order over the
    factors) and the census of the output is users x live items.  Peak: B 4 GiB / 16 GiB."""
    rt = rfm[3]
    k = 1024
    imap = wt.id_map(map_name)
    assert pt.pad4(k) == imap.width == k
    A, LU, B, LI, c = pt.operands(wt.PAIR_USERS, imap.m, k)
    want = pt.scores(rfm, A, LU, B, LI, c)
    wt.assert_room(rt, imap.n * (k + 1) * 8 + wt.PAIR_USERS * imap.n * 8)
    Bw = wt.wide_table(rt, imap.n, k, imap.wide, B)
    LIw = wt.wide_table(rt, imap.n, None, imap.wide, LI)
    imap.assert_sizes(Bw.numel())
    _announce(imap, f"rfm_pair_scores, B wide ({map_name})")
    out = _wide_scores(rt, A, LU, Bw, LIw, c, imap.n)
    got = wt.live_rows(out.t(), imap.wide).T
    assert np.isfinite(want).all() and (want > 1e-6).mean() > 0.8 and (want < 1 - 1e-6).mean() > 0.8
    wt.assert_same_bits(got, want, "scores of the live items")
    assert wt.census(out) == wt.PAIR_USERS * imap.m
    wt.assert_census(Bw, imap.m, "B after rfm_pair_scores")
    wt.assert_census(LIw, imap.m, "LI after rfm_pair_scores")


def test_side_sums_wide_v_and_wide_a(rfm):
    """rfm_fm_side_sums at k = 1 024 reading a wide V (the side matrix's columns under the map:
    ``V[col * k + f]``) and writing a wide A (its rows under a map of their own, every other row of
    the wide side matrix empty: ``A[r * kpad + f]``).  The launch writes EVERY row of A and L -- an
    empty row's sums are zero -- so the census of A is the whole table, its non-zero elements are as
    many as the compact call's, and the live rows are the compact call's bit for bit.
    Peak: V and A, 8 GiB."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    rt = rfm[3]
    k = 1024
    X = pt.side_matrix()
    w, V = pt.side_parameters(k)
    cmap, rmap = wt.id_map("fm-V-k1024"), wt.id_map("pair-A-kpad1024")
    assert cmap.m == X.n_cols and rmap.m == X.n_rows and pt.pad4(k) == k
    want_A, want_L = pt.side_sums(rfm, X, w, V)
    wt.assert_room(rt, 2 * cmap.n * (k + 1) * 8)
    Vw = wt.wide_table(rt, cmap.n, k, cmap.wide, V)
    ww = wt.wide_table(rt, cmap.n, None, cmap.wide, w)
    cmap.assert_sizes(Vw.numel())
    _announce(cmap, "rfm_fm_side_sums, V wide")
    lens = torch.zeros(rmap.n, dtype=torch.int64, device=rt.torch_device)
    lens[torch.from_numpy(rmap.wide).to(rt.torch_device)] = rt.upload(np.diff(X.indptr))
    indptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=rt.torch_device), lens.cumsum(0)])
    assert int(indptr[-1]) == len(X.indices)
    indices, data = rt.upload(cmap(X.indices).astype(np.int32)), rt.upload(np.array(X.data))
    A, L = wt.nan_table(rt, (rmap.n, k)), wt.nan_table(rt, (rmap.n,))
    rmap.assert_sizes(A.numel())
    _announce(rmap, "rfm_fm_side_sums, A wide")
    _lib.check(rt.lib.rfm_fm_side_sums(rt.ctx, indptr.data_ptr(), indices.data_ptr(), data.data_ptr(), rmap.n,
                                       ww.data_ptr(), Vw.data_ptr(), cmap.n, k, A.data_ptr(), L.data_ptr()))
    rt.sync()
    wt.assert_same_bits(wt.live_rows(A, rmap.wide), want_A, "A")
    wt.assert_same_bits(wt.live_rows(L, rmap.wide), want_L, "L")
    assert wt.census(A) == A.numel() and wt.census(L) == L.numel(), "a row of the wide A or L was not written"
    assert wt.count_nonzero(A) == int(np.count_nonzero(want_A)) > 0
    assert wt.count_nonzero(L) == int(np.count_nonzero(want_L))
    wt.assert_census(Vw, cmap.m, "V after rfm_fm_side_sums")


def test_pair_scores_wide_output(rfm):
    """rfm_pair_scores into a wide OUTPUT at the smallest operand width, kpad = 4: 133 selected users x
    4.2 M items, ``out[s * n_items + item]`` past 2^32 bytes from user 128 on.  Nothing is compact here:
    the wide output is compared on the device with the same call on the two halves of the items,
    whose outputs stay below the threshold.  Peak: the output 4.2 GiB and its halves, 8.4 GiB."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    rt = rfm[3]
    k, n_items, n_sel = 4, wt.WIDE_OUT_ITEMS, wt.WIDE_OUT_SEL
    assert n_sel == 133 and n_sel * n_items * 8 > 2 ** 32 > (n_sel - wt.MARGIN - 1) * n_items * 8
    wt.assert_room(rt, 2 * n_sel * n_items * 8)
    print(f"\nrfm_pair_scores, output wide: {n_sel} users x {n_items} items = {n_sel * n_items * 8 / GIB:.3f} GiB; "
          f"crossed T32b at user {n_sel - wt.MARGIN}")
    gen = torch.Generator(device=rt.torch_device).manual_seed(5)
    B = 0.5 * torch.randn((n_items, k), generator=gen, dtype=torch.float64, device=rt.torch_device)
    LI = 0.5 * torch.randn((n_items,), generator=gen, dtype=torch.float64, device=rt.torch_device)
    A, LU, _, _, c = pt.operands(n_sel + 4, 8, k)
    user_ids = np.arange(n_sel, dtype=np.int32)[::-1].copy() + 2   # (a selection: the last users first)
    dA, dLU, dc = rt.upload(pt._padded(A)), rt.upload(np.array(LU)), rt.upload(np.array([c]))
    d_ids = rt.upload(user_ids)

    def call(first, count):
        out = wt.nan_table(rt, (n_sel * count + pt.GUARD,))
        _lib.check(rt.lib.rfm_pair_scores(rt.ctx, dA.data_ptr(), dLU.data_ptr(), A.shape[0], d_ids.data_ptr(), n_sel,
                                          B[first:].data_ptr(), LI[first:].data_ptr(), count, k, dc.data_ptr(),
                                          out.data_ptr()))
        rt.sync()
        assert bool(out[n_sel * count:].isnan().all()), "an element past the output was written"
        return out[: n_sel * count].view(n_sel, count)

    whole = call(0, n_items)
    assert wt.census(whole) == n_sel * n_items
    half = (n_items // 2 // 64) * 64 + 64   # (a whole number of item tiles: the halves' tiles are the whole's)
    for first, count in ((0, half), (half, n_items - half)):
        assert n_sel * count * 8 < 2 ** 32
        part = call(first, count)
        assert torch.equal(whole[:, first: first + count], part), f"items {first} .. {first + count}"
        del part
    top = whole[n_sel - wt.MARGIN:, :].cpu().numpy()   # the rows past the threshold hold scores of their own
    assert ((top > 1e-6) & (top < 1 - 1e-6)).mean() > 0.8 and len(np.unique(top[:, :1000])) > 4000


def _pair_call(rt, name, A, LU, user_ids, Bw, LIw, n_items, c, *rest):
    """An rfm_pair_* entry on a wide B that is on the device: the eleven arguments they share, no
    exclusion lists, then `rest`."""
    from relevance_factorizationmachine_amd import _lib
    dA, dLU, dc = rt.upload(pt._padded(A)), rt.upload(np.array(LU)), rt.upload(np.array([c]))
    ids = rt.upload(np.asarray(user_ids, dtype=np.int32))
    _lib.check(getattr(rt.lib, name)(rt.ctx, dA.data_ptr(), dLU.data_ptr(), A.shape[0], ids.data_ptr(), len(user_ids),
                                     Bw.data_ptr(), LIw.data_ptr(), n_items, A.shape[1], dc.data_ptr(), None, None,
                                     *rest))
    rt.sync()


def test_pair_lists_on_a_wide_b(rfm):
    """rfm_pair_topk, rfm_pair_ranks_n and rfm_pair_order against a wide B (kpad = 1 024, 0.5 M items;
    a guard item's logit is NaN and a NaN logit is never ranked): the best items and the targets are
    the live items past T, lists and ranks are the compact call's with the items under the map, the
    scores bit for bit.  rfm_pair_order runs a selection of 1 029 users (five users, repeated) at
    depth 8 with every selected user in one block, so its logit workspace (block rows x items) is
    past 4 GiB as well.  Peak: B 4 GiB and the workspace 4.3 GiB."""
    import torch
    _, _, recommend, rt = rfm
    k = 1024
    imap = wt.id_map("pair-B-kpad1024")
    T, m, n = imap.top, imap.m, imap.n
    A, LU, B, LI, c = pt.operands(wt.PAIR_USERS, m, k)
    LI = np.array(LI)
    high = np.arange(imap.compact(T - 1), m)
    LI[high] += 6.0                                   # the best items of every user: the ids from T - 1 on
    users = np.array([4, 0, 2, 2, 1, 3], dtype=np.int32)
    K, depth, n_order = 9, 8, (1 << 10) + 5
    tgt_items_c = np.concatenate([[0, 5] + high.tolist()] * len(users)).astype(np.int32)   # (ascending; T - 1 .. n - 1)
    tgt_indptr = np.arange(len(users) + 1, dtype=np.int64) * 6
    order_users = (np.arange(n_order) % wt.PAIR_USERS).astype(np.int32)
    c_top = pt.topk(rfm, A, LU, B, LI, c, K, user_ids=users)
    c_ranks = pt.ranks(rfm, A, LU, B, LI, c, tgt_indptr, tgt_items_c, user_ids=users)
    c_order = pt.order(rfm, A, LU, B, LI, c, depth, user_ids=order_users)
    assert len(high) == 4 and (c_top[0][:, :4] >= high[0]).all() and (c_ranks[2] == m).all()

    ws_order = recommend.order_workspace_bytes(n_order, n, depth)[1]
    assert ws_order >= n_order * n * 8 > 2 ** 32
    wt.assert_room(rt, n * (k + 1) * 8 + ws_order)
    Bw = wt.wide_table(rt, n, k, imap.wide, B)
    LIw = wt.wide_table(rt, n, None, imap.wide, LI)
    imap.assert_sizes(Bw.numel())
    _announce(imap, "rfm_pair_topk / rfm_pair_ranks_n / rfm_pair_order, B wide")
    print(f"rfm_pair_order workspace: {ws_order / GIB:.3f} GiB for {n_order} selected users x {n} items")
    dev = rt.torch_device

    def blank(shape, dtype):
        return pt._filled(rt, shape, dtype)

    ws = blank((recommend.topk_workspace_bytes(len(users), n, K),), torch.uint8)
    items, scores = blank((len(users), K), torch.int32), blank((len(users), K), torch.float64)
    _pair_call(rt, "rfm_pair_topk", A, LU, users, Bw, LIw, n, c, K, ws.data_ptr(), items.data_ptr(), scores.data_ptr())
    np.testing.assert_array_equal(items.cpu().numpy(), imap(c_top[0]))
    wt.assert_same_bits(scores.cpu().numpy(), c_top[1], "top-K scores")

    n_tgt = len(tgt_items_c)
    ws = blank((recommend.ranks_workspace_bytes(len(users), n, n_tgt),), torch.uint8)
    ranks, rscores = blank((n_tgt,), torch.int32), blank((n_tgt,), torch.float64)
    cand = blank((len(users),), torch.int32)
    d_ti, d_tx = rt.upload(tgt_indptr), rt.upload(imap(tgt_items_c).astype(np.int32))
    _pair_call(rt, "rfm_pair_ranks_n", A, LU, users, Bw, LIw, n, c, d_ti.data_ptr(), d_tx.data_ptr(), n_tgt,
               ws.data_ptr(), ranks.data_ptr(), rscores.data_ptr(), cand.data_ptr())
    np.testing.assert_array_equal(ranks.cpu().numpy(), c_ranks[0])
    wt.assert_same_bits(rscores.cpu().numpy(), c_ranks[1], "scores of the targets")
    np.testing.assert_array_equal(cand.cpu().numpy(), c_ranks[2])
    del ws

    ws = torch.empty((ws_order,), dtype=torch.uint8, device=dev)
    items, scores = blank((n_order, depth), torch.int32), blank((n_order, depth), torch.float64)
    n_ranked = blank((n_order,), torch.int32)
    _pair_call(rt, "rfm_pair_order", A, LU, order_users, Bw, LIw, n, c, depth, ws.data_ptr(), ws_order,
               items.data_ptr(), scores.data_ptr(), n_ranked.data_ptr())
    np.testing.assert_array_equal(items.cpu().numpy(), imap(c_order[0]))
    wt.assert_same_bits(scores.cpu().numpy(), c_order[1], "scores of the ordered items")
    np.testing.assert_array_equal(n_ranked.cpu().numpy(), c_order[2])
    assert (c_order[2] == m).all()
    wt.assert_census(Bw, m, "B after the list entries")
    wt.assert_census(LIw, m, "LI after the list entries")


def test_rows_normalise_on_a_wide_table(rfm):
    """rfm_rows_normalise (the neighbours' row normalisation, ``M + r * ld``) of a wide table at
    k = 1 024 into a wide output.  Every row is read: a guard row's norm is NaN and so is its output
    row, so the census of the output and of the norms is the live rows'.  Peak: M and the output, 8 GiB."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    rt = rfm[3]
    k = 1024
    imap = wt.id_map("pair-B-kpad1024")
    M = np.array(pt.operands(wt.PAIR_USERS, imap.m, k)[2])

    def call(d_M, n):
        out, norm = wt.nan_table(rt, (n, k)), wt.nan_table(rt, (n,))
        _lib.check(rt.lib.rfm_rows_normalise(rt.ctx, d_M.data_ptr(), n, k, k, out.data_ptr(), norm.data_ptr()))
        rt.sync()
        return out, norm

    c_out, c_norm = (t.cpu().numpy() for t in call(rt.upload(M), imap.m))
    assert np.isfinite(c_out).all() and (c_norm > 0).all()
    wt.assert_room(rt, 2 * imap.n * (k + 1) * 8)
    Mw = wt.wide_table(rt, imap.n, k, imap.wide, M)
    imap.assert_sizes(Mw.numel())
    _announce(imap, "rfm_rows_normalise, M and its output wide")
    out, norm = call(Mw, imap.n)
    wt.assert_same_bits(wt.live_rows(out, imap.wide), c_out, "normalised rows")
    wt.assert_same_bits(wt.live_rows(norm, imap.wide), c_norm, "norms")
    wt.assert_census(out, imap.m, "the normalised table")
    wt.assert_census(norm, imap.m, "the norms")
    wt.assert_census(Mw, imap.m, "M after rfm_rows_normalise")


def test_mf_fold_in_fixed_side_wide(rt):
    """rfm_mf_fold_in at k = 128 with the FIXED side wide (``F + j * k``: the examples' ids under the
    map); the new rows keep their compact size.  Fold-in claims a fixed order: bit for bit.
    Peak: F 4 GiB."""
    import fold_in_common as fi
    import torch
    from relevance_factorizationmachine_amd import _lib
    case = fi.shape_case(128)
    k = case.k
    imap = wt.id_map("mf-fold-F-k128")
    assert (imap.m, imap.width) == (case.n_fixed, k)
    want_rows, want_bias = fi.run_fold(rt, case)
    F, fb = case.fixed()
    x0, c0 = case.start()
    ids = imap(case.ids)
    assert (ids >= imap.top).any() and (ids < imap.top).any()
    wt.assert_room(rt, imap.n * (k + 1) * 8)
    Fw, fbw = wt.wide_table(rt, imap.n, k, imap.wide, F), wt.wide_table(rt, imap.n, None, imap.wide, fb)
    imap.assert_sizes(Fw.numel())
    _announce(imap, "rfm_mf_fold_in, the fixed side wide")
    d_ptr, d_ids, d_order = rt.upload(case.row_ptr), rt.upload(ids.astype(np.int32)), rt.upload(case.order)
    d_ry, d_rows, d_bias = rt.upload(case.ry()), rt.upload(x0), rt.upload(c0)
    _lib.check(rt.lib.rfm_mf_fold_in(rt.ctx, d_ptr.data_ptr(), d_ids.data_ptr(), d_ry.data_ptr(), d_order.data_ptr(),
                                     case.n_new, Fw.data_ptr(), fbw.data_ptr(), imap.n, ms.B0, k, ms.LR, ms.REG,
                                     case.n_passes, d_rows.data_ptr(), d_bias.data_ptr()))
    rt.sync()
    wt.assert_same_bits(d_rows.cpu().numpy(), want_rows, "the folded rows")
    wt.assert_same_bits(d_bias.cpu().numpy(), want_bias, "the folded biases")
    assert not np.array_equal(want_rows, x0)
    wt.assert_census(Fw, imap.m, "F after rfm_mf_fold_in")
    wt.assert_census(fbw, imap.m, "the fixed bias after rfm_mf_fold_in")
    for a, b in ((wt.live_rows(Fw, imap.wide), F), (wt.live_rows(fbw, imap.wide), fb)):
        wt.assert_same_bits(a, b, "the fixed side")


def test_fm_step_generic_forward_on_row_blocks(rt):
    """The step's forward in the generic kernel on the plan's padded row blocks (``ell + r * ell_stride``
    in front of the gather of V) at 64 lanes per row: k = 128, a log whose rows hold at most 16 entries,
    the smallest batch of the many-rows shape.  Hot mode -1: every sum has a fixed order, the column at
    T is a split column, so the step is the compact run's bit for bit.  Peak: V 4 GiB."""
    k, map_name, hot = 128, "fm-V-k128-bounded", -1
    n_rows = fr.many_rows_minimum(rt, k, True)
    assert n_rows <= gf.GRAD_TOL_ROWS and gf.fixed_order(k, hot)
    imap, log, theta, full, wlog = _fm_case(map_name, k, n_rows, True)
    got = []
    for lg in (log, wlog):
        dev = gf.DeviceLog(rt, lg, k, n_rows, hot)
        try:
            form = dev.plan.step_form(n_rows)
            assert dev.plan.layout()["row_blocks"] == 1 and dev.plan.layout()["lanes_per_row"] == _lpr(k) == 64
            assert form["kind"] == "blocks" and form["lanes8"] == 0, form
            assert form["lanes"] == 64 and form["block"] == 1024, form
            print(f"step form: {form}")
            if lg is wlog:
                assert _assert_hot_state(dev, imap, hot, n_rows, k) == "split"
                params = _wide_params(rt, imap, theta, f"rfm_fm_step, generic forward on row blocks, {n_rows} rows")
            else:
                params = gf.Params(rt, *theta)
            gf.step(dev, full, params, STEP_LR)
            if lg is wlog:
                params.assert_census("after rfm_fm_step")
            got.append(params.live() if lg is wlog else params.host())
        finally:
            dev.close()
    at = imap.compact(imap.top)
    assert not np.array_equal(got[0][2][at], theta[2][at])
    for name, a, b in zip(("w0", "w", "V"), got[1], got[0]):
        wt.assert_same_bits(a, b, name)


def _wide_fold_ints(rt, case, rmap):
    """row_ptr [n + 1] and order [n] of a fold-in whose new rows are the case's under the map, every
    other row without an example, built on the device: the order is the case's rule (descending
    example count, stable)."""
    import torch
    dev = rt.torch_device
    lens = torch.zeros(rmap.n, dtype=torch.int64, device=dev)
    lens[torch.from_numpy(rmap.wide).to(dev)] = rt.upload(case.lengths)
    row_ptr = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), lens.cumsum(0)])
    order = torch.argsort(-lens, stable=True).to(torch.int32)
    head = order[: case.n_new].cpu().numpy()
    busy = int((case.lengths > 0).sum())
    np.testing.assert_array_equal(head[:busy], rmap(case.order[:busy]))
    assert int(row_ptr[-1]) == int(case.lengths.sum())
    return row_ptr, order


def test_fm_fold_in_new_rows_wide(rt):
    """rfm_fm_fold_in at k = 1 024 with the NEW side wide: g, V_new and A_new of 0.5 M rows each, l,
    w_new and L_new beside them (``g + r * kpad``, ``V_new + r * k``, ``A_new + r * kpad``); the
    case's eight rows sit at the live ids, every other row has no example and NaN inputs, so it
    leaves NaN.  Fold-in has a fixed order: bit for bit.  Peak: three tables, 12 GiB."""
    import fm_fold_common as ff
    from relevance_factorizationmachine_amd import _lib
    case = ff.pass_case(1024, 2)
    k = case.k
    rmap = wt.id_map("fm-fold-new-k1024")
    assert (rmap.m, rmap.width) == (case.n_new, k) and ff.pad4(k) == k
    assert (case.lengths[rmap.compact(rmap.top):] > 0).any(), "no row past T has an example"
    want_V, want_w, want_A, want_L = ff.run_fold(rt, case)
    F, fL = case.fixed()
    g, l = case.feature_sums()
    nu0, om0 = case.start()
    wt.assert_room(rt, 3 * rmap.n * (k + 1) * 8)
    tabs = {name: wt.wide_table(rt, rmap.n, None if a.ndim == 1 else k, rmap.wide, a)
            for name, a in (("g", g), ("l", l), ("V", nu0), ("w", om0))}
    A, L = wt.nan_table(rt, (rmap.n, k)), wt.nan_table(rt, (rmap.n,))
    rmap.assert_sizes(tabs["V"].numel())
    _announce(rmap, "rfm_fm_fold_in, g, V_new and A_new wide")
    row_ptr, order = _wide_fold_ints(rt, case, rmap)
    d_ids, d_ry = rt.upload(case.ids), rt.upload(case.ry())
    d_F, d_fL, d_c = rt.upload(F), rt.upload(fL), rt.upload(np.array([ff.C0]))
    _lib.check(rt.lib.rfm_fm_fold_in(
        rt.ctx, row_ptr.data_ptr(), d_ids.data_ptr(), d_ry.data_ptr(), order.data_ptr(), rmap.n, tabs["g"].data_ptr(),
        tabs["l"].data_ptr(), d_F.data_ptr(), d_fL.data_ptr(), case.n_fixed, d_c.data_ptr(), k, case.lr, case.n_passes,
        tabs["w"].data_ptr(), tabs["V"].data_ptr(), A.data_ptr(), L.data_ptr()))
    rt.sync()
    for name, t, want in (("V_new", tabs["V"], want_V), ("w_new", tabs["w"], want_w), ("A_new", A, want_A),
                          ("L_new", L, want_L), ("g", tabs["g"], g), ("l", tabs["l"], l)):
        wt.assert_same_bits(wt.live_rows(t, rmap.wide), want, name)
        wt.assert_census(t, rmap.m, f"{name} after rfm_fm_fold_in")
    assert not np.array_equal(want_V, nu0)


def test_mf_fold_in_new_rows_wide(rt):
    """rfm_mf_fold_in at k = 128 with the NEW rows wide (``rows + r * k`` and the bias beside them, 4.2 M
    rows; the fixed side compact): the other side of test_mf_fold_in_fixed_side_wide.  Peak: 4 GiB."""
    import fold_in_common as fi
    from relevance_factorizationmachine_amd import _lib
    case = fi.shape_case(128)
    k = case.k
    rmap = wt.id_map("mf-fold-new-k128")
    assert (rmap.m, rmap.width) == (case.n_new, k)
    assert (case.lengths[rmap.compact(rmap.top):] > 0).any(), "no row past T has an example"
    want_rows, want_bias = fi.run_fold(rt, case)
    F, fb = case.fixed()
    x0, c0 = case.start()
    wt.assert_room(rt, rmap.n * (k + 1) * 8)
    rows, bias = wt.wide_table(rt, rmap.n, k, rmap.wide, x0), wt.wide_table(rt, rmap.n, None, rmap.wide, c0)
    rmap.assert_sizes(rows.numel())
    _announce(rmap, "rfm_mf_fold_in, the new rows wide")
    row_ptr, order = _wide_fold_ints(rt, case, rmap)
    d_ids, d_ry, d_F, d_fb = rt.upload(case.ids), rt.upload(case.ry()), rt.upload(F), rt.upload(fb)
    _lib.check(rt.lib.rfm_mf_fold_in(rt.ctx, row_ptr.data_ptr(), d_ids.data_ptr(), d_ry.data_ptr(), order.data_ptr(),
                                     rmap.n, d_F.data_ptr(), d_fb.data_ptr(), case.n_fixed, ms.B0, k, ms.LR, ms.REG,
                                     case.n_passes, rows.data_ptr(), bias.data_ptr()))
    rt.sync()
    wt.assert_same_bits(wt.live_rows(rows, rmap.wide), want_rows, "the folded rows")
    wt.assert_same_bits(wt.live_rows(bias, rmap.wide), want_bias, "the folded biases")
    wt.assert_census(rows, rmap.m, "the new rows after rfm_mf_fold_in")
    wt.assert_census(bias, rmap.m, "the new biases after rfm_mf_fold_in")
    assert not np.array_equal(want_rows, x0)


def test_pair_lists_by_item_on_wide_tables(rfm):
    """The audience form -- rfm_pair_topk_by_item, rfm_pair_ranks_by_item, rfm_pair_order_by_item: the
    rows of the tile are items, its columns users -- at kpad = 1 024 with BOTH tables wide: the queries
    are item ids on either side of T in a wide B, the candidates the users of a wide A, whose guard
    rows give NaN logits that are never ranked.  The best users and the targets are the live users
    from T - 1 on.  Lists and ranks are the compact call's with the users under the map, the values
    bit for bit.  Peak: A and B, 8 GiB."""
    import audience_common as au
    import torch
    from relevance_factorizationmachine_amd import _lib
    rt = rfm[3]
    k = 1024
    umap, imap = wt.id_map("audience-A-kpad1024"), wt.id_map("audience-B-kpad1024")
    A, LU, B, LI, c = pt.operands(umap.m, imap.m, k)
    LU = np.array(LU)
    high = np.arange(umap.compact(umap.top - 1), umap.m)
    LU[high] += 6.0                                    # every item's best users: the ids from T - 1 on
    sel = np.array([imap.m - 1, 0, imap.compact(imap.top), imap.compact(imap.top), imap.compact(imap.top - 1), 2],
                   dtype=np.int32)
    K, depth = 9, 12
    tgt_users = np.concatenate([[0, 5] + high.tolist()] * len(sel)).astype(np.int32)
    tgt_indptr = np.arange(len(sel) + 1, dtype=np.int64) * (2 + len(high))
    c_top = au.topk_by_item(rfm, A, LU, B, LI, c, K, item_ids=sel, raw=False)
    c_ranks = au.ranks_by_item(rfm, A, LU, B, LI, c, tgt_indptr, tgt_users, item_ids=sel)
    c_order = au.order_by_item(rfm, A, LU, B, LI, c, depth, item_ids=sel)
    assert len(high) == 4 and (c_top[0][:, :3] >= high[0]).all() and (c_ranks[2] == umap.m).all()

    wt.assert_room(rt, (umap.n + imap.n) * (k + 1) * 8)
    dev = (wt.wide_table(rt, umap.n, k, umap.wide, A), wt.wide_table(rt, umap.n, None, umap.wide, LU),
           wt.wide_table(rt, imap.n, k, imap.wide, B), wt.wide_table(rt, imap.n, None, imap.wide, LI),
           rt.upload(np.array([c], dtype=np.float64)))
    umap.assert_sizes(dev[0].numel())
    imap.assert_sizes(dev[2].numel())
    _announce(umap, "the by-item entries, A wide")
    _announce(imap, "the by-item entries, B wide")
    n_sel, w_sel = len(sel), imap(sel).astype(np.int32)
    args, keep = au._lead(rt, dev, umap.n, w_sel, n_sel, imap.n, k, None)

    def mapped(users):
        return np.where(users >= 0, umap(np.maximum(users, 0)), -1)

    ws, _ = au._workspace(rt, "rfm_pair_topk_workspace", n_sel, umap.n, K)
    users, values = au._guarded(rt, n_sel * K, torch.int32), au._guarded(rt, n_sel * K, torch.float64)
    _lib.check(rt.lib.rfm_pair_topk_by_item(*args, K, 0, ws.data_ptr(), users.data_ptr(), values.data_ptr()))
    rt.sync()
    np.testing.assert_array_equal(au._take(users, n_sel * K, (n_sel, K)), mapped(c_top[0]))
    wt.assert_same_bits(au._take(values, n_sel * K, (n_sel, K)), c_top[1], "top-K values")

    n_tgt = len(tgt_users)
    d_ti, d_tx = rt.upload(tgt_indptr), rt.upload(umap(tgt_users).astype(np.int32))
    ws, _ = au._workspace(rt, "rfm_pair_ranks_workspace", n_sel, umap.n, n_tgt)
    ranks, scores = au._guarded(rt, n_tgt, torch.int32), au._guarded(rt, n_tgt, torch.float64)
    cand = au._guarded(rt, n_sel, torch.int32)
    _lib.check(rt.lib.rfm_pair_ranks_by_item(*args, d_ti.data_ptr(), d_tx.data_ptr(), n_tgt, ws.data_ptr(),
                                             ranks.data_ptr(), scores.data_ptr(), cand.data_ptr()))
    rt.sync()
    np.testing.assert_array_equal(au._take(ranks, n_tgt, (n_tgt,)), c_ranks[0])
    wt.assert_same_bits(au._take(scores, n_tgt, (n_tgt,)), c_ranks[1], "scores of the targets")
    np.testing.assert_array_equal(au._take(cand, n_sel, (n_sel,)), c_ranks[2])

    ws, ws_bytes = au._workspace(rt, "rfm_pair_order_workspace", n_sel, umap.n, depth)
    users, scores = au._guarded(rt, n_sel * depth, torch.int32), au._guarded(rt, n_sel * depth, torch.float64)
    n_ranked = au._guarded(rt, n_sel, torch.int32)
    _lib.check(rt.lib.rfm_pair_order_by_item(*args, depth, ws.data_ptr(), ws_bytes, users.data_ptr(), scores.data_ptr(),
                                             n_ranked.data_ptr()))
    rt.sync()
    np.testing.assert_array_equal(au._take(users, n_sel * depth, (n_sel, depth)), mapped(c_order[0]))
    wt.assert_same_bits(au._take(scores, n_sel * depth, (n_sel, depth)), c_order[1], "scores of the ordered users")
    np.testing.assert_array_equal(au._take(n_ranked, n_sel, (n_sel,)), c_order[2])
    for name, t, m in (("A", dev[0], umap), ("LU", dev[1], umap), ("B", dev[2], imap), ("LI", dev[3], imap)):
        wt.assert_census(t, m.m, f"{name} after the by-item entries")
