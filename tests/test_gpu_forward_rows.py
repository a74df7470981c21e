"""The FM forward (fm_forward_kernel) row by row against the long-double oracle of
forward_rows_common.py, at every (lanes per row, vector width, chunks per lane) class, in both
workgroup shapes, through every way the log is read, in every loss form of rfm_fm_train, and at the
edges of a workgroup's trip.  Needs an MI355X: ``pytest -m gpu``.

Every test asks the library which shape or form a call takes (rfm_fm_forward_geometry,
rfm_fm_train_forms; part D the step's kernel and form, rfm_fm_step_form) and asserts it before it compares anything; sizes -- the smallest row count of
the many-rows shape, the rows of a trip, of a pass of the grid -- come from those queries, not
from a CU count written here.  Tolerances (logit, score, loss) are the derived ones of
forward_rows_common.py.

A  rfm_fm_forward, every class x both shapes: scores row by row; bit-identical scores of a log row
   wherever it appears in a launch and across launches of one shape; a non-finite row of V.
   The second pass of the grid is covered where it needs at most 150 000 rows: at 256 CUs that is
   every class (131 073 rows at 4 lanes per row).  The one-row shape never takes a second pass
   through this call: a log long enough for one takes the many-rows shape.
B  rfm_fm_forward_loss, both shapes (the many-rows one stages its logarithms through LDS).
C  every loss form of rfm_fm_train, by calls with lr = 0 (the parameters keep their bits, so the
   oracle of an iteration is one long-double pass over its rows).
D  the training forward's many-rows shape per class, through the gradient forms."""
import functools

import numpy as np
import pytest

import forward_rows_common as fr
import grad_forms_common as gf

pytestmark = pytest.mark.gpu

LD = np.longdouble
BIG, SMALL = 1024, 256
SECOND_PASS_MAX_ROWS = 150_000
KS = sorted(gf.CLASS_OF)
IDS = [gf.class_id(k) for k in KS]


@pytest.fixture(scope="module")
def rt():
    from relevance_factorizationmachine_amd import runtime
    return runtime.Runtime.get()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def _geo(k, records):
    """What the geometry query says of a factor count: lanes per row, rows of a trip and lane
    groups of both shapes, the workgroups of a full grid, the many-rows minimum."""
    from relevance_factorizationmachine_amd import runtime
    rt = runtime.Runtime.get()
    big, small = fr.forward_geometry(rt, 1 << 22, k, records), fr.forward_geometry(rt, 1, k, records)
    assert big["block"] == BIG and small["block"] == SMALL and big["lpr"] == small["lpr"]
    lpr = big["lpr"]
    assert small["trip"] == SMALL // lpr and big["trip"] % (BIG // lpr) == 0
    m = fr.many_rows_minimum(rt, k, records)
    assert fr.forward_geometry(rt, m - 1, k, records)["block"] == SMALL
    return {"lpr": lpr, "T": big["trip"], "G": BIG // lpr, "R": big["trip"] // (BIG // lpr), "T1": small["trip"],
            "grid": big["grid"], "min": m}


def _assert_shape(rt, n, k, records, block):
    geo = fr.forward_geometry(rt, n, k, records)
    assert geo["block"] == block, (n, k, geo)
    return geo


# --------------------------------------------------------------------------
# A. rfm_fm_forward: every class x both shapes, row by row
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case_a(k):
    """Row counts of both shapes for a factor count, and ONE log that holds them all as prefixes:
    the last row of every count is empty, the long row sits beside an empty row in flight with it
    (many-rows shape: rows m T + g and m T + G + g of a lane group; one row in flight: the next
    lane group's row)."""
    g = _geo(k, False)
    T, G, T1, m = g["T"], g["G"], g["T1"], g["min"]
    n_a = -(-m // T) * T + 1                      # a trip multiple + 1
    n_b, n_c = g["grid"] * T, g["grid"] * T + 1    # one pass of the grid, one pass + 1
    assert n_a < n_b
    second = n_c <= SECOND_PASS_MAX_ROWS
    many = (n_a, n_b, n_c) if second else (n_a, n_a + T)
    m1 = (min(m - 1, 1500) - 1) // T1
    one = ((m1 - 1) * T1 + 1, m1 * T1, m1 * T1 + 1)
    assert one[-1] < m and one[0] > 2 * T + 6  # (the rows of `pairs` lie inside every launch)
    pairs = ((T + 3, T + G + 3) if g["R"] >= 2 else (T + 3, T + 4), (2 * T + 5, 2 * T + 6))
    empties = tuple(sorted({n - 1 for n in many + one}))
    log, theta, o = fr.case(k, max(many), empties, pairs)
    # (at least 80 % of the rows unsaturated, in the log and in every prefix of it that is launched)
    assert min(fr.unsaturated_share(o.take(slice(0, n))) for n in many + one) >= 0.8
    return {"many": many, "one": one, "second": second, "log": log, "theta": theta, "o": o, "geo": g}


@functools.lru_cache(maxsize=None)
def _device_a(k):
    from relevance_factorizationmachine_amd import runtime
    return fr.DeviceRows(runtime.Runtime.get(), _case_a(k)["log"])


def _id_lists(rng, n, n_log, long_row):
    """Row ids of a launch of n rows on a log of n_log > n rows: a permutation of the first n rows, a
    strict subset of the log in no order, and ids with repeats (neighbouring positions, far
    positions, the long row and an empty row among them)."""
    perm = rng.permutation(n).astype(np.int32)
    subset = rng.permutation(n_log)[:n].astype(np.int32)
    rep = rng.integers(0, n_log, size=n).astype(np.int32)
    rep[[0, 1, n // 2, n - 1]] = long_row
    rep[[2, 3, n - 2]] = 0
    rep[5:9] = rep[4]
    return {"a permutation": perm, "a strict subset": subset, "ids with repeats": rep}


@pytest.mark.parametrize("shape", ["many", "one"])
@pytest.mark.parametrize("k", KS, ids=IDS)
def test_forward_scores_row_by_row(rt, k, shape):
    c = _case_a(k)
    o, g, counts = c["o"], c["geo"], c[shape]
    block = BIG if shape == "many" else SMALL
    dev, params = _device_a(k), gf.Params(rt, *c["theta"])
    assert o.length[0] == 0 and o.length[c["log"]["features"].shape[0] - 1] == 0
    cols = c["log"]["features"].indices
    assert cols.min() == 0 and cols.max() == dev.n - 1  # column 0 and the last column are in use
    base = None
    for n in sorted(counts, reverse=True):
        geo = _assert_shape(rt, n, k, False, block)
        if shape == "many" and c["second"]:  # only one pass + 1 makes a workgroup take a second trip
            assert (geo["grid"] * geo["trip"] < n) == (n == counts[-1]), (n, geo)
        assert o.length[n - 1] == 0
        got = fr.forward(rt, dev, params, n)
        fr.assert_scores(got, o.take(slice(0, n)), k, f"{n} rows")
        if base is None:
            base = got
        # a row's score does not depend on the rows of the launch or on its neighbours
        np.testing.assert_array_equal(_bits(got), _bits(base[:n]), err_msg=f"{n} rows against {len(base)}")
    n = counts[0]
    long_row = g["T"] + 3
    assert o.length[long_row] == 5 * g["lpr"] + 3 and o.length[g["T"] + (g["G"] if g["R"] >= 2 else 1) + 3] == 0
    for name, ids in _id_lists(np.random.default_rng(k), n, len(base), long_row).items():
        _assert_shape(rt, len(ids), k, False, block)
        got = fr.forward(rt, dev, params, len(ids), ids)
        fr.assert_scores(got, o.take(ids), k, name)
        # the same log row scores the same bits at every position, in every launch of the shape
        np.testing.assert_array_equal(_bits(got), _bits(base[ids]), err_msg=name)


@pytest.mark.parametrize("shape", ["many", "one"])
def test_forward_with_a_non_finite_row_of_V(rt, shape):
    """The V row of the column of entry 0 of the log is non-finite: the rows that hold the column
    score non-finite, every other row meets the tolerance, and the empty rows -- whose padding
    reads entry 0 -- score what they score with a finite V, to the bit."""
    k = 32
    c = _case_a(k)
    n = c[shape][0]
    X = c["log"]["features"]
    col = int(X.indices[0])
    w0, w, V = c["theta"]
    V_bad = V.copy()
    V_bad[col, ::2], V_bad[col, 1::2] = np.nan, np.inf
    with np.errstate(invalid="ignore"):
        o_bad = fr.row_oracle(X[:n], w0, w, V_bad)
    holds = np.zeros(n, dtype=bool)
    holds[np.unique(np.repeat(np.arange(n), np.diff(X.indptr[: n + 1]))[X.indices[: X.indptr[n]] == col])] = True
    np.testing.assert_array_equal(~np.isfinite(o_bad.p), holds)
    assert 10 < holds.sum() < n // 2
    _assert_shape(rt, n, k, False, BIG if shape == "many" else SMALL)
    dev = _device_a(k)
    good = fr.forward(rt, dev, gf.Params(rt, w0, w, V), n)
    got = fr.forward(rt, dev, gf.Params(rt, w0, w, V_bad), n)
    fr.assert_scores(got, o_bad, k, "non-finite row of V")  # (finite exactly where the oracle is)
    empty = c["o"].length[:n] == 0
    assert empty.sum() > 10 and empty[0] and empty[n - 1]
    np.testing.assert_array_equal(_bits(got[empty]), _bits(good[empty]))
    assert len(np.unique(_bits(got[empty]))) == 1
    sig_w0 = fr.Rows(np.array([LD(w0[0])]), np.array([LD(abs(w0[0]))]), np.array([0]))
    fr.assert_scores(got[empty][:1], sig_w0, k, "sigmoid(w0)")
    np.testing.assert_array_equal(_bits(got[~holds]), _bits(good[~holds]))


# --------------------------------------------------------------------------
# B. rfm_fm_forward_loss, both shapes
# --------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["many", "one"])
@pytest.mark.parametrize("k", fr.LOSS_CLASSES, ids=[gf.class_id(k) for k in fr.LOSS_CLASSES])
def test_forward_loss_at_the_edges_of_a_trip(rt, k, shape):
    """Row counts of a trip multiple - 1, + 0, + 1 (the many-rows shape: its last trip's stage
    holds one slot without a row, none, all but one), with and without row ids, with d_out_pred
    given and NULL."""
    c = _case_a(k)
    g, o, log = c["geo"], c["o"], c["log"]
    if shape == "many":
        T, block = g["T"], BIG
        m = -(-(g["min"] + 1) // T)
    else:
        T, block = g["T1"], SMALL
        m = (min(g["min"] - 1, 1500) - 1) // T
    n_log = log["features"].shape[0]
    dev, params = _device_a(k), gf.Params(rt, *c["theta"])
    rng = np.random.default_rng(100 + k)
    for n in (m * T - 1, m * T, m * T + 1):
        assert n <= n_log
        geo = _assert_shape(rt, n, k, False, block)
        assert geo["trip"] == T
        for ids in (None, rng.permutation(n_log)[:n].astype(np.int32)):
            rows = slice(0, n) if ids is None else ids
            want, tol = fr.loss_oracle(o.take(rows), k, log["labels"][rows], log["pscores"][rows])
            for with_pred in (True, False):
                what = (f"{n} rows, ids {'given' if ids is not None else 'none'}, "
                        f"pred {'given' if with_pred else 'NULL'}")
                loss, pred = fr.forward_loss(rt, dev, params, n, ids, with_pred)
                fr.assert_loss(loss, want, tol, what)
                if with_pred:
                    fr.assert_scores(pred, o.take(rows), k, what)


# --------------------------------------------------------------------------
# C. every loss form of rfm_fm_train, by calls with lr = 0
# --------------------------------------------------------------------------
def _train_case(k, n_train, n_val, lpr=None, max_len=None):
    """(log, theta, oracle) of a training log and of a validation log under the same parameters."""
    tr = fr.case(k, n_train, (), (), max_len, 11, lpr)
    va = fr.case(k, n_val, (), (), max_len, 12, lpr)
    assert all(np.array_equal(a, b) for a, b in zip(tr[1], va[1]))
    assert fr.unsaturated_share(tr[2]) >= 0.8 and fr.unsaturated_share(va[2]) >= 0.8
    return tr, va


def _batches(rng, n_train, batch, n_iters):
    """Distinct ids within an iteration, another subset each iteration; every second iteration
    without the rows past the clip and near +-40 (rows 1 .. 8), whose loss terms carry the widest
    tolerance."""
    ids = np.empty((n_iters, batch), dtype=np.int32)
    for it in range(n_iters):
        pool = np.arange(n_train) if it % 2 else np.concatenate([[0], np.arange(9, n_train)])
        ids[it] = rng.permutation(pool)[:batch]
    return ids


def _check_losses(tl, vl, ids, tr, va, k, want_train=True, want_val=True):
    (log, _, o), (vlog, _, vo) = tr, va
    if want_val:
        want, tol = fr.loss_oracle(vo, k, vlog["labels"], vlog["pscores"])
        for it in range(len(ids)):
            fr.assert_loss(vl[it], want, tol, f"validation loss of iteration {it}")
    if want_train:
        for it, b in enumerate(ids):
            want, tol = fr.loss_oracle(o.take(b), k, log["labels"][b], log["pscores"][b])
            fr.assert_loss(tl[it], want, tol, f"train loss of iteration {it}")


def _run_form(rt, k, tr, va, batch, n_iters, expect, max_batch=None, hot=0, register=False, part=None, check=None):
    """One rfm_fm_train call with lr = 0: asserts the forms the library reports for it (``expect``:
    a subset of FORM_NAMES -> value), runs it, holds its losses to the oracle.  Returns the losses."""
    from relevance_factorizationmachine_amd import _lib
    dev = gf.DeviceLog(rt, tr[0], k, max_batch or batch, hot)
    try:
        val = fr.DeviceRows(rt, va[0])
        if register:
            _lib.check(rt.lib.rfm_fm_plan_register_log(rt.ctx, dev.plan.handle, 0, *val.csr_ptrs(), val.n_rows))
        if check:
            check(dev)
        forms = fr.train_forms(rt, dev.plan, batch, n_iters, part or 0, val, val.n_rows)
        for name, value in expect.items():
            assert forms[name] == value, (name, forms)
        ids = _batches(np.random.default_rng(k + batch), dev.n_rows, batch, n_iters)
        tl, vl = fr.train_lr0(rt, dev, gf.Params(rt, *tr[1]), ids, val, part)
        _check_losses(tl, vl, ids, tr, va, k)
        return tl, vl
    finally:
        dev.close()


PLAIN = {"sliced": 0, "merged": 0}


def test_train_in_forward_logarithms_one_row_shape(rt):
    tr, va = _train_case(16, 600, 100)
    _run_form(rt, 16, tr, va, 64, 3,
              dict(PLAIN, scores_only=0, ride=0, ride_val=0, train_block=SMALL, val_block=SMALL))


def test_train_in_forward_logarithms_many_rows_shape(rt, monkeypatch):
    """RFM_DEFER_LOSS=0 at a batch of the many-rows minimum: the train-loss forward stages its
    logarithms through LDS, reading the plan's row and entry records."""
    k = 128
    batch = _geo(k, True)["min"]
    tr, va = _train_case(k, batch + 40, 100)
    monkeypatch.setenv("RFM_DEFER_LOSS", "0")
    _run_form(rt, k, tr, va, batch, 4, dict(PLAIN, scores_only=0, ride=0, train_block=BIG, val_block=SMALL),
              check=lambda dev: dev.plan.layout()["row_blocks"] == 0 or pytest.fail("the plan holds row blocks"))


def test_train_deferred_scores_launches_apart(rt, monkeypatch):
    tr, va = _train_case(16, 600, 100)
    monkeypatch.setenv("RFM_RIDE_LOSS", "0")
    _run_form(rt, 16, tr, va, 64, 5,
              dict(PLAIN, scores_only=1, ride=0, ride_val=0, train_block=SMALL, val_block=SMALL))


@pytest.mark.parametrize("k", [16, 200])
def test_train_riding_train_rows_on_a_records_plan(rt, k):
    tr, va = _train_case(k, 600, 100)
    _run_form(rt, k, tr, va, 64, 5, dict(PLAIN, scores_only=1, ride=1, ride_val=0, train_block=SMALL),
              check=lambda dev: dev.plan.layout()["row_blocks"] == 0 or pytest.fail("the plan holds row blocks"))


def test_train_riding_train_rows_on_a_row_block_plan(rt):
    """max_batch at the many-rows size, every row within one round of a lane group, the call's batch
    small: the riders form reading padded row blocks (FwdKind::kBlocksRiders)."""
    k = 32
    g = _geo(k, True)
    tr, va = _train_case(k, g["min"] + 10, 100, max_len=g["lpr"])
    _run_form(rt, k, tr, va, 64, 5, dict(PLAIN, scores_only=1, ride=1, ride_val=0, train_block=SMALL),
              max_batch=g["min"],
              check=lambda dev: dev.plan.layout()["row_blocks"] == 1 or pytest.fail("the plan holds no row blocks"))


def test_train_riding_validation_rows(rt):
    """The validation log registered in slot 0 rides too; the same arrays unregistered do not, and
    give the same losses."""
    k = 16
    tr, va = _train_case(k, 600, 100)
    on = _run_form(rt, k, tr, va, 64, 5, dict(PLAIN, scores_only=1, ride=1, ride_val=1, val_block=SMALL),
                   register=True)
    off = _run_form(rt, k, tr, va, 64, 5, dict(PLAIN, scores_only=1, ride=1, ride_val=0, val_block=SMALL))
    _, tol = fr.loss_oracle(va[2], k, va[0]["labels"], va[0]["pscores"])
    assert (np.abs(on[1] - off[1]) <= 2 * float(tol)).all()  # (both are inside tol of the oracle)


def test_train_fixed_order_plan_does_not_ride(rt):
    k, batch = 32, 1024
    tr, va = _train_case(k, 1500, 100)

    def hot_class(dev):
        assert dev.plan.info()["hot_columns"] > 0

    _run_form(rt, k, tr, va, batch, 5, dict(PLAIN, scores_only=1, ride=0, ride_val=0), hot=-2, check=hot_class)
    _run_form(rt, k, tr, va, batch, 5, dict(PLAIN, scores_only=1, ride=1), hot=0, check=hot_class)


def test_train_130_iterations_cross_the_run_with_riding_rows(rt):
    tr, va = _train_case(16, 600, 100)
    _run_form(rt, 16, tr, va, 48, 130, dict(PLAIN, scores_only=1, ride=1, run_len=128))


@pytest.mark.parametrize("k,mode", [(130, None), (16, "2")])
def test_train_merged_launch(rt, monkeypatch, k, mode):
    """Both losses in one launch of the many-rows shape (FwdKind::kCsrPair): batch + validation rows at the
    many-rows minimum, the batch odd and no multiple of the trip -- the boundary between the two
    logs falls inside a trip and, with two rows in flight, between a lane group's two rows."""
    g = _geo(k, False)
    T, G, R = g["T"], g["G"], g["R"]
    batch = 60 * T + (G if R == 2 else 0) + 3
    n_val = g["min"] - batch + 9
    assert batch % 2 == 1 and batch % T and n_val > T and batch + n_val >= g["min"]
    _assert_shape(rt, batch + n_val, k, False, BIG)
    if mode is not None:
        monkeypatch.setenv("RFM_MERGE_LOSS", mode)
    tr, va = _train_case(k, batch + 50, n_val, lpr=g["lpr"])
    _run_form(rt, k, tr, va, batch, 2,
              dict(sliced=0, merged=1, scores_only=0, ride=0, train_block=BIG, val_block=BIG))


@pytest.mark.parametrize("k", [130, 300, 600])
def test_train_sliced_form(rt, monkeypatch, k):
    monkeypatch.setenv("RFM_SLICED_MIN_ROWS", "1")
    tr, va = _train_case(k, 300, 30, lpr=64)
    _run_form(rt, k, tr, va, 40, 3, dict(sliced=1, merged=0, scores_only=0, ride=0),
              check=lambda dev: dev.plan.sliced()["slices"] > 0 or pytest.fail("the plan has no slices"))


def test_train_part_takes_the_long_calls_form(rt):
    k = 16
    tr, va = _train_case(k, 600, 100)
    dev = gf.DeviceLog(rt, tr[0], k, 64)
    try:
        val = fr.DeviceRows(rt, va[0])
        assert fr.train_forms(rt, dev.plan, 64, 1, 0, val, 100)["scores_only"] == 0  # rfm_fm_train of one iteration
    finally:
        dev.close()
    _run_form(rt, k, tr, va, 64, 1, dict(PLAIN, scores_only=1, ride=1), part=5)


# --------------------------------------------------------------------------
# D. the training forward's many-rows shape, per class, through the gradient
# --------------------------------------------------------------------------
RARE = 8


@functools.lru_cache(maxsize=None)
def _case_d(k, blocks):
    """Batch = the class's many-rows minimum + one trip + 1, on a log of as many rows; the oracle
    gradients of the full batch and of a five-row shard: computed once, shared by the hot modes.
    These logs carry no rows past the clip (A to C cover it): their x, in the thousands, would
    dwarf every other term of a column's sums."""
    g = _geo(k, True)
    batch = g["min"] + g["T"] + 1
    max_len = g["lpr"] if blocks else 2 * g["lpr"] + 1
    log, theta, o = fr.case(k, batch, (), (), max_len, 21, None, RARE, 0)
    assert o.length.max() == max_len and fr.unsaturated_share(o) >= 0.8
    full = np.random.default_rng(k).permutation(batch).astype(np.int32)
    shard = np.array([11, 0, batch // 2, 42, batch - 3], dtype=np.int32)  # row 0 is empty
    return log, theta, full, shard, gf.grad_oracle(log, full, *theta), gf.grad_oracle(log, shard, *theta)


@pytest.mark.parametrize("hot", [0, -1, -2])
@pytest.mark.parametrize("layout", ["blocks", "records"])
@pytest.mark.parametrize("k", KS, ids=IDS)
def test_training_forward_many_rows_through_the_gradient(rt, k, layout, hot):
    g = _geo(k, True)
    log, theta, full, shard, o_full, o_shard = _case_d(k, layout == "blocks")
    dev = gf.DeviceLog(rt, log, k, len(full), hot)
    try:
        lay, info = dev.plan.layout(), dev.plan.info()
        assert lay["row_blocks"] == (layout == "blocks") and lay["lanes_per_row"] == g["lpr"]
        assert lay["longest_row"] == (g["lpr"] if layout == "blocks" else 2 * g["lpr"] + 1)
        _assert_shape(rt, len(full), k, True, BIG)
        _assert_shape(rt, len(shard), k, True, SMALL)  # the shard: the one-row shape on the same layout
        assert info["forward_workgroups"] == fr.forward_geometry(rt, len(full), k, True)["grid"] <= g["grid"]
        # the hot class the case is meant for: -2 means -1 where the many-rows shape has no
        # fixed-order sums (several chunks per lane, or fewer than 16 lanes per row)
        chunked = gf.chunked(k)
        want_hot = not chunked and (hot == 0 or (hot == -2 and g["lpr"] >= 16))
        assert (info["hot_columns"] > 0) == want_hot, info
        assert info["hot_columns"] <= dev.n - RARE  # the rare columns stay in the sparse class
        # the kernel and form of the step's forward (rfm_fm_step_form): the layout's kind, fixed-order
        # where the plan sums a hot class so; the 8-lane kernel at k = 32 on row blocks otherwise
        fixed = hot == -2 and want_hot
        kind = layout + ("_fixed" if fixed else "")
        lanes8 = k == 32 and layout == "blocks" and not fixed
        form, small = dev.plan.step_form(len(full)), dev.plan.step_form(len(shard))
        assert (form["block"], form["kind"], form["fixed_order"], form["lanes8"]) == (BIG, kind, int(fixed), int(lanes8)), form
        assert form["lanes"] == (8 if lanes8 else g["lpr"]) and form["trip"] == g["T"], form
        assert form["workgroups"] == info["forward_workgroups"], form
        assert (small["block"], small["kind"], small["lanes8"], small["lanes"]) == (SMALL, kind, 0, g["lpr"]), small
        gf.check_all_forms(dev, gf.Params(rt, *theta), full, shard, o_full, o_shard, gf.fixed_order(k, hot))
    finally:
        dev.close()
