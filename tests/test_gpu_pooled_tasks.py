"""The gradient launch deals the marked slots of a workgroup evenly to its lane groups (DESIGN 4,
item 2): group g of GPB sums the positions [g * per, (g + 1) * per) of the workgroup's T marks in
slot order, per = ceil(T / GPB) -- its part -- and which columns cross a part's edges is read off
the marks.  A workgroup in which one task has more marks than a group's list holds (WIN: 16 / 32 / 64
at 4 / 8 / >= 16 lanes per row) runs its tasks as they are; so does every workgroup of a plan whose
tasks expect no more than one batch of four marks (small batches; every plan here expects more,
`Marks` asserts it).  Needs an MI355X: ``pytest -m gpu``.

Every case builds its log so that the marks fall where the case needs them, REPLAYS the plan's slot
layout on the host (`_slots`: the sparse-class columns in ascending order, a column that does not
fit into the rest of a workgroup's slots starts at the next workgroup) and asserts, from the marks
per task and per workgroup, that the case is what it claims before it trusts it; the replay itself
is held to the plan's slot and task counts.  These assertions check the CONSTRUCTION of a case --
that its marks fall so that the kernel's rule sends the workgroup down the path the case is meant
for -- not the kernel's decision: nothing observed on the device tells the paths apart, the results
hold on both.  Gradients, records and one in-place step are held to
the long-double oracle with the derived bounds of grad_forms_common.py (`grad_tol`, `step_bound`);
bit equality is asked only between calls of the same kernel on the same inputs."""
import functools

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import grad_forms_common as gf

pytestmark = pytest.mark.gpu

STEP_LR = 2.0 ** -3  # an update the size of the parameters
KS = [8, 16, 32, 64, 128, 13, 33]  # every single-chunk class (lanes per row 4 ... 64, both widths)


@pytest.fixture(scope="module")
def rt():
    from relevance_factorizationmachine_amd import runtime
    return runtime.Runtime.get()


def _device_log(rt, log, k, max_batch, hot):
    dev = gf.DeviceLog(rt, log, k, max_batch, hot)
    dev.plan_max_batch = max_batch
    return dev


def _win(k):
    """Slots a lane group lists before it runs the chain."""
    return {4: 16, 8: 32}.get(gf.CLASS_OF[k][0], 64)


def _gpb(k):
    return 256 // gf.CLASS_OF[k][0]


# --------------------------------------------------------------------------
# the replay of the plan's slot layout
# --------------------------------------------------------------------------
def _slots(X, k, task_words, hot_cols=()):
    """(row of every slot or -1, column of every slot or -1, slots of a task, of a workgroup)."""
    C = 64 * task_words
    BC = _gpb(k) * C
    Xc = X.tocsc()
    Xc.sort_indices()
    hot = set(int(c) for c in hot_cols)
    at, pieces = 0, []
    for c in range(X.shape[1]):
        rows = Xc.indices[Xc.indptr[c]: Xc.indptr[c + 1]]
        if c in hot or len(rows) == 0:
            continue
        if len(rows) <= BC:
            if len(rows) > BC - at % BC:
                at += BC - at % BC
            pieces.append((at, c, rows))
            at += len(rows)
        else:
            at = -(-at // BC) * BC
            pieces.append((at, c, rows))
            at += -(-len(rows) // BC) * BC
    n_slots = max(1, -(-at // BC)) * BC
    slot_row = np.full(n_slots, -1, dtype=np.int64)
    slot_col = np.full(n_slots, -1, dtype=np.int64)
    for start, c, rows in pieces:
        slot_row[start: start + len(rows)] = rows
        slot_col[start: start + len(rows)] = c
    return slot_row, slot_col, C, BC


class Marks:
    """What a batch marks on a plan, from the replay: marks per task and per workgroup, and for
    every workgroup the part (lane group) of each of its marks with the mark's column."""

    def __init__(self, dev, k, ids):
        info = dev.plan.info()
        row, col, C, BC = _slots(dev.X, k, info["task_words"], dev.plan.hot_columns())
        assert len(row) == info["slots"] and len(row) // C == info["tasks"], (len(row), C, info)
        marked = np.isin(row, np.asarray(ids)) & (row >= 0)
        self.per_task = marked.reshape(-1, C).sum(axis=1)
        self.per_wg = marked.reshape(-1, BC).sum(axis=1)
        self.task_of_wg = self.per_task.reshape(-1, _gpb(k))
        self.over = (self.task_of_wg > _win(k)).any(axis=1)  # workgroups that run their tasks as they are
        # the plan deals marks evenly at all: a task expects more than one batch of four marks
        assert C * dev.plan_max_batch > 4 * dev.n_rows, (C, dev.plan_max_batch, dev.n_rows)
        self.pooled = ~self.over  # workgroups whose marks are dealt evenly
        self.cols_of_wg = [col[b * BC: (b + 1) * BC][marked[b * BC: (b + 1) * BC]] for b in range(len(self.per_wg))]
        self.gpb = _gpb(k)

    def parts(self, b):
        """Part of every mark of workgroup b."""
        T = int(self.per_wg[b])
        per = -(-T // self.gpb)
        return np.arange(T) // max(per, 1)

    def through_parts(self, b):
        """Parts of workgroup b that lie inside one column which goes on on both sides."""
        cols, parts = self.cols_of_wg[b], self.parts(b)
        n = 0
        for g in np.unique(parts):
            i = np.flatnonzero(parts == g)
            if i[0] > 0 and i[-1] + 1 < len(cols) and len(np.unique(cols[i[0] - 1: i[-1] + 2])) == 1:
                n += 1
        return n

    def widest_column_spread(self, b):
        """Most parts between the first and the last mark of one column of workgroup b."""
        cols, parts = self.cols_of_wg[b], self.parts(b)
        return max((int(parts[cols == c][-1] - parts[cols == c][0]) for c in np.unique(cols)), default=0)


# --------------------------------------------------------------------------
# the checks every case runs
# --------------------------------------------------------------------------
def _check_case(rt, dev, k, ids, theta, oracle, fixed, what):
    """Dense gradient, records, dense again and records again on one plan (interleaved), then two
    in-place steps from the same parameters: everything against the oracle, and -- where every sum
    has a fixed order -- the second call of each form bit for bit the first."""
    hot_cols = dev.plan.hot_columns()
    params = gf.Params(rt, *theta)
    g1, _ = gf.dense_grad(dev, ids, params)
    r1 = gf.grad_rows(dev, ids, params, dev.n)
    g2, _ = gf.dense_grad(dev, ids, params)
    r2 = gf.grad_rows(dev, ids, params, dev.n)
    touched = gf.check_dense(g1, dev, ids, oracle, hot_cols, f"{what} dense")
    gf.check_records(r1, g1, dev, touched, hot_cols, fixed, f"{what} records")
    if fixed:
        np.testing.assert_array_equal(g2, g1, err_msg=f"{what}: two dense gradients differ")
        np.testing.assert_array_equal(r2.rec, r1.rec, err_msg=f"{what}: two record lists differ")
        assert r2.count == r1.count and r2.gw0 == r1.gw0
    else:
        gf.check_dense(g2, dev, ids, oracle, hot_cols, f"{what} dense, second call")
    got = []
    for _ in range(2):
        p = gf.Params(rt, *theta)
        gf.step(dev, ids, p, STEP_LR)
        got.append(p.host())
    for name, ratio in zip(("w0", "w", "V"), gf.step_excess(got[0], theta, oracle, STEP_LR, len(ids))):
        print(f"{what} {name}: worst |got - (theta - lr g)| / bound = {float(ratio.max()):.3g}")
        assert (ratio <= 1).all(), (what, name, np.argwhere(ratio > 1)[:5], float(ratio.max()))
    if fixed:
        for a, b in zip(got[0], got[1]):
            np.testing.assert_array_equal(a, b, err_msg=f"{what}: two steps differ")


# --------------------------------------------------------------------------
# 1. part edges inside columns: every list exactly full
# --------------------------------------------------------------------------
def _run_lengths(k):
    """Marks per column: 1, 2, WIN - 1, WIN, WIN + 1, 3 WIN + 5, repeated until the columns fill
    more than one workgroup (the last one partly)."""
    win = _win(k)
    unit = [1, 2, win - 1, win, win + 1, 3 * win + 5]
    reps = -(-(_gpb(k) * win + win) // sum(unit))
    return unit * reps


@functools.lru_cache(maxsize=None)
def _full_lists_case(k):
    """Column c holds the rows 0 .. stride * m_c - 1, stride = 64 / WIN, and the batch is every
    stride-th row: a column starts on a multiple of the stride, so exactly every stride-th slot is
    marked -- WIN marks in every 64-slot task that the columns fill -- and column c has m_c marks."""
    stride = 64 // _win(k)
    lens = [stride * m for m in _run_lengths(k)]
    n_rows, n = max(lens), len(lens)
    rng = np.random.default_rng(100 + k)
    D = np.zeros((n_rows, n))
    for c, lc in enumerate(lens):
        D[:lc, c] = rng.standard_normal(lc)
    log = {"features": csr_matrix(D), "labels": (rng.random(n_rows) < 0.5).astype(np.int64),
           "pscores": rng.uniform(0.1, 1.0, size=n_rows) ** 0.5}
    theta = gf.perturbed_init(k, n, k)
    ids = rng.permutation(np.arange(0, n_rows, stride)).astype(np.int32)
    return log, theta, ids, gf.grad_oracle(log, ids, *theta)


CASES_1 = [(k, -1) for k in KS] + [(32, 0)]


@pytest.mark.parametrize("k,hot", CASES_1, ids=[f"{gf.class_id(k)}-hot{hot}" for k, hot in CASES_1])
def test_part_edges_inside_columns(rt, k, hot):
    """Every list exactly full (per = WIN in the workgroups the columns fill: every plane of the
    parked records in use, a part = a task's marks, the columns start, end and pass through parts)
    and a last workgroup that the columns fill partly (its parts are not its tasks)."""
    log, theta, ids, oracle = _full_lists_case(k)
    win, gpb = _win(k), _gpb(k)
    dev = _device_log(rt, log, k, len(ids), hot)
    try:
        assert dev.plan.layout()["lanes_per_row"] == gf.CLASS_OF[k][0]
        assert dev.plan.info()["task_words"] == 1
        assert (dev.plan.info()["hot_columns"] > 0) == (hot == 0)
        m = Marks(dev, k, ids)
        assert m.pooled.all() and m.per_wg[-1] > 0
        if hot == -1:
            assert len(m.per_wg) >= 2
            # every list exactly full, but for the slots a workgroup's last columns leave free
            assert (m.task_of_wg[0, : gpb // 2] == win).all() and m.per_wg[0] > (gpb - 4) * win
            # a part of the first workgroup: (nearly) a whole list, every plane of parked records in use
            planes = {4: 4, 8: 4, 16: 4, 32: 2, 64: 1}[gf.CLASS_OF[k][0]]
            assert -(-m.per_wg[0] // gpb) > win - win // planes
            assert m.per_wg[-1] % gpb != 0 and m.through_parts(len(m.per_wg) - 1) >= 1
            assert max(m.widest_column_spread(b) for b in range(len(m.per_wg))) >= 3
        _check_case(rt, dev, k, ids, theta, oracle, hot == -1, f"full lists k={k} hot={hot}")
    finally:
        dev.close()


# --------------------------------------------------------------------------
# 2. few marks: T = 1, GPB - 1, GPB, a multiple of GPB and one less (T = 0 beside them); a column
#    over distant parts
# --------------------------------------------------------------------------
N_LONE = 6  # rows that only column 2 holds


@functools.lru_cache(maxsize=None)
def _few_marks_log(k):
    """The columns of case 1 at stride 1 (column c = the rows 0 .. m_c - 1) until they fill more
    than one workgroup, on a plan whose batch may be the whole log (a task is one word); then UNIT
    rows, one entry each, dealt round robin to the columns of the first workgroup but its last few: a
    batch of t of them marks exactly t slots there, a few per task; then N_LONE rows that only
    column 2 holds (the column's last slots).  Returns the log, parameters, the unit rows, the lone rows."""
    win, gpb = _win(k), _gpb(k)
    unit = [1, 2, win - 1, win, win + 1, 3 * win + 5]
    lens = unit * -(-(gpb * 64 + win) // sum(unit))
    fit = int(np.searchsorted(np.cumsum(lens), gpb * 64, side="right"))  # columns inside workgroup 0
    n_base, n = max(lens), len(lens)
    n_unit = 3 * gpb + 8
    home = np.arange(n_unit) % max(4, fit - 7)  # (the columns grow: the last ones may move out)
    n_rows = n_base + n_unit + N_LONE
    rng = np.random.default_rng(200 + k)
    D = np.zeros((n_rows, n))
    for c, lc in enumerate(lens):
        D[:lc, c] = rng.standard_normal(lc)
    units = n_base + np.arange(n_unit)
    D[units, home] = rng.standard_normal(n_unit)
    lone = n_base + n_unit + np.arange(N_LONE)
    D[lone, 2] = rng.standard_normal(N_LONE)
    log = {"features": csr_matrix(D), "labels": (rng.random(n_rows) < 0.5).astype(np.int64),
           "pscores": rng.uniform(0.1, 1.0, size=n_rows) ** 0.5}
    return log, gf.perturbed_init(k + 1, n, k), units, lone


def _batch_of(want, units, lone):
    """A batch that marks `want` slots of workgroup 0: the lone rows (a run of marks in one column
    and one task) and unit rows for the rest."""
    # (every other unit row first: the batch is not a prefix of a column's rows)
    order = np.concatenate([units[::2], units[1::2]])
    n_lone = min(want, len(lone))
    return np.concatenate([lone[:n_lone], order[: want - n_lone]]).astype(np.int32)


@pytest.mark.parametrize("k", KS, ids=[gf.class_id(k) for k in KS])
def test_few_marks(rt, k):
    log, theta, units, lone = _few_marks_log(k)
    n_rows = log["features"].shape[0]
    gpb = _gpb(k)
    dev = _device_log(rt, log, k, n_rows, -1)
    try:
        assert dev.plan.info()["task_words"] == 1
        assert len(Marks(dev, k, np.arange(n_rows)).per_wg) >= 2
        for want in (1, gpb - 1, gpb, 3 * gpb, 3 * gpb - 1):
            ids = _batch_of(want, units, lone)
            m = Marks(dev, k, ids)
            # (the workgroups behind the first are without marks: T = 0 there)
            assert m.per_wg[0] == want and (m.per_wg[1:] == 0).all() and not m.over.any(), (want, m.per_wg)
            assert m.pooled.all()
            _check_case(rt, dev, k, ids, theta, gf.grad_oracle(log, ids, *theta), True, f"T={want} k={k}")
        # a column whose marks land in parts several groups apart: T = 6, all in column 2, a mark per
        # part (two at 4 groups)
        m = Marks(dev, k, lone)
        assert m.per_wg[0] == N_LONE and m.per_wg.sum() == N_LONE and m.pooled[0]
        assert m.widest_column_spread(0) == (N_LONE - 1 if gpb >= N_LONE else 2)
        _check_case(rt, dev, k, lone.astype(np.int32), theta, gf.grad_oracle(log, lone, *theta), True, f"spread k={k}")
    finally:
        dev.close()


def test_a_workgroup_without_marks(rt):
    """T = 0: the rows of the batch are in the columns of the first workgroup only."""
    k = 32
    gpb, rng = _gpb(k), np.random.default_rng(5)
    n_rows, first = 300, 20
    D = np.zeros((n_rows, 60))
    D[:150, :first] = rng.standard_normal((150, first))  # 3 000 slots: workgroups 0 to 2
    D[150:, first:] = rng.standard_normal((150, 60 - first)) * (rng.random((150, 60 - first)) < 0.5)
    log = {"features": csr_matrix(D), "labels": (rng.random(n_rows) < 0.5).astype(np.int64),
           "pscores": rng.uniform(0.1, 1.0, size=n_rows) ** 0.5}
    theta = gf.perturbed_init(9, 60, k)
    dev = _device_log(rt, log, k, n_rows, -1)
    try:
        ids = rng.permutation(np.arange(150, n_rows))[:40].astype(np.int32)
        m = Marks(dev, k, ids)
        assert m.per_wg[0] == 0 and m.per_wg.max() > gpb and not m.over.any() and m.pooled.any()
        _check_case(rt, dev, k, ids, theta, gf.grad_oracle(log, ids, *theta), True, "T=0")
    finally:
        dev.close()


# --------------------------------------------------------------------------
# 3. split columns: a workgroup inside one column, its partial row, the finalize launch
# --------------------------------------------------------------------------
@pytest.mark.parametrize("k", [8, 33, 128], ids=[gf.class_id(k) for k in (8, 33, 128)])
def test_split_columns(rt, k):
    bc = gf.full_batch_workgroup_slots(k)
    n_rows = bc + 37
    log, theta, full, _ = gf.split_case(k, n_rows, 24 if n_rows > 3000 else 60, 1, 11 * k)
    dev = _device_log(rt, log, k, n_rows, -1)
    try:
        assert dev.geometry()["BC"] == bc and dev.partial_rows(0) == 2
        assert dev.plan.info()["split_columns"] >= 1
        # the whole log: the split column's workgroups overflow at fewer than 16 lanes per row
        # (64 marks in every task) and are pooled from 16 on; a sixteenth of it: pooled everywhere
        for ids in (full, full[: n_rows // 16]):
            m = Marks(dev, k, ids)
            assert m.over[0] == (len(ids) == n_rows and _win(k) < 64), (m.task_of_wg[0], _win(k))
            assert m.pooled[0] == (not m.over[0])
            _check_case(rt, dev, k, ids, theta, gf.grad_oracle(log, ids, *theta), True, f"split k={k} B={len(ids)}")
    finally:
        dev.close()


# --------------------------------------------------------------------------
# 4. overflow: one workgroup runs its tasks as they are, its neighbour is pooled
# --------------------------------------------------------------------------
@pytest.mark.parametrize("k,m_cols,r_rows,density,max_batch", [(32, 5, 26, 0.05, 64), (8, 2, 17, 0.12, 128)],
                         ids=["lpr16-k32", "lpr4-k8"])
def test_overflow_fallback_beside_a_pooled_workgroup(rt, k, m_cols, r_rows, density, max_batch):
    """m adjacent columns held by exactly the same r rows, all of them in the batch: L = m r
    consecutive marked slots.  With L >= 2 WIN + 2 and L <= the slots of a task, any task edge
    leaves more than WIN of them in one task."""
    n_rows, n = 4096, 48  # (4 lanes per row: 128 rows per step, so that a task expects 8 marks, not 4)
    rng = np.random.default_rng(40 + k)
    D = rng.standard_normal((n_rows, n)) * (rng.random((n_rows, n)) < density)  # (two workgroups' slots)
    block = np.arange(20, 20 + m_cols)
    held = np.sort(rng.choice(n_rows, size=r_rows, replace=False))
    D[:, block] = 0.0
    D[np.ix_(held, block)] = rng.standard_normal((r_rows, m_cols))
    log = {"features": csr_matrix(D), "labels": (rng.random(n_rows) < 0.5).astype(np.int64),
           "pscores": rng.uniform(0.1, 1.0, size=n_rows) ** 0.5}
    theta = gf.perturbed_init(k + 2, n, k)
    rest = np.setdiff1d(np.arange(n_rows), held)
    ids = rng.permutation(np.concatenate([held, rng.choice(rest, size=max_batch - r_rows, replace=False)])).astype(np.int32)
    dev = _device_log(rt, log, k, max_batch, -1)
    try:
        win, words = _win(k), dev.plan.info()["task_words"]
        L = m_cols * r_rows
        assert L >= 2 * win + 2 and L <= 64 * words, (L, win, words)
        m = Marks(dev, k, ids)
        assert m.over.sum() == 1 and len(m.over) >= 2, m.per_task.max()
        b = int(np.argmax(m.over))
        beside = b + 1 if b + 1 < len(m.over) else b - 1
        assert m.pooled[beside] and m.per_wg[beside] > 0
        _check_case(rt, dev, k, ids, theta, gf.grad_oracle(log, ids, *theta), True, f"overflow k={k}")
    finally:
        dev.close()
