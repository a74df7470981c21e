"""The step's forward at 8 lanes x 4 factors per row (fm_forward_lanes8_kernel<1024>: k = 20, 24,
28, 32 on padded row blocks, many-rows shape, arrival-order hot sums).  Needs an MI355X: ``pytest -m gpu``.
Every test asks the library which kernel and form a step on its plan takes (rfm_fm_step_form) and asserts
it before it compares anything: a launch condition that stopped taking the 8-lane kernel would leave
every bit below as it is.

What the kernel leaves -- the Q rows, the residuals, the marks -- stays inside the plan: the C ABI shows
it through the gradient.  The sums of the sparse class run over the marked slots in slot order
(fm_consume_kernel), and g_w0 over the forward workgroups' residual sums in thread order, so they are
functions of those bits alone.  The ORDER-EXACT reference of a row is therefore the 16-lane map
itself, which this shape has to reproduce bit for bit:

- the same batch on a plan of fixed-order hot sums (hot_min_count -2: fm_forward_kernel<16, 2, 1, 1024,
  kBlocksFixed>, the 16-lane map at two rows per lane group), and
- pieces of the batch small enough for the one-row shape on the SAME plan (<16, 2, 1, 256, kBlocks>).

In the logs of the bit tests every row that is not empty holds a column of its own (below the shared
columns in even rows: its first entry; above them in odd rows: its last), so G_V and g_w of that
column are err x (q - V x) and err x of ONE row: every row's Q row, residual and mark is held on its
own, and a mark that is missing, doubled or at another slot moves a column by a whole term.  The
columns shared by many rows and g_w0 are compared bit for bit as well.  The hot columns (arrival
order: no bits to compare) and every other element are held to the long-double oracle of
grad_forms_common within grad_tol(B) * S, on logs of 96 columns, whose dense oracle fits memory; one
in-place step under SGD within step_bound and one under AdaGrad within adagrad_common's intervals.

Sizes come from rfm_fm_forward_geometry: the smallest batch of the many-rows shape (every workgroup
one trip), that batch + 1 (a last workgroup of one row: lane groups without a row), and one pass of
the full grid + 1 (workgroup 0 makes a second trip of one row, every other workgroup none).  Row
lengths 0, 1, 8, 9, 15, 16 -- no entry, one lane, the last first-entry, the first second-entry, one
short of the block, the block -- are at least a twentieth of every log each (asserted)."""
import functools

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import adagrad_common as ac
import forward_rows_common as fr
import grad_forms_common as gf

pytestmark = pytest.mark.gpu

BIG, SMALL = 1024, 256
N_HOT, N_SHARED = 24, 40   # shared columns: the first 24 frequent (hot: ranks 0 - 15 on the tile, 16 - 23 walked)
N_PLAIN = 96               # columns of a log without private columns
EDGES = (0, 1, 8, 9, 15, 16)
STEP_LR = 2.0 ** -3


@pytest.fixture(scope="module")
def rt():
    from relevance_factorizationmachine_amd import runtime
    return runtime.Runtime.get()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@functools.lru_cache(maxsize=None)
def _sizes(k):
    from relevance_factorizationmachine_amd import runtime
    rt = runtime.Runtime.get()
    big = fr.forward_geometry(rt, 1 << 22, k, True)
    m = fr.many_rows_minimum(rt, k, True)
    assert big["block"] == BIG and big["lpr"] == 16 and big["trip"] == 128  # (the geometry is the 16-lane map's)
    return {"min": m, "plus_one": m + 1, "second_trip": big["grid"] * big["trip"] + 1, "T": big["trip"]}


@functools.lru_cache(maxsize=None)
def _log(B, private, every_row=False, longest=16, seed=0):
    """B rows of 0 .. 16 entries (a sixth of them at each length of EDGES), ascending columns.  Shared
    column c is drawn with weight 1 - c / 26 (c < N_HOT), 0.01 (the others); shared column 0 is in every
    row that has a shared entry (`every_row`: in every row, and no row is empty).  `private`: the last
    entry a row draws is a column of its own.  `longest` > 16: row 7 gets that many entries."""
    rng = np.random.default_rng(77 + seed + B + 2 * private)
    lens = np.where(rng.random(B) < 0.5, rng.choice(EDGES, size=B), rng.integers(2, 17, size=B))
    if every_row:
        lens = np.maximum(lens, 1 if not private else 2)
    if longest > 16:
        lens[7] = longest
    n_sh = N_SHARED if private else N_PLAIN - 1  # (a plain log's last column is in no row)
    weight = np.full(n_sh, 0.01)
    weight[:N_HOT] = 1.0 - np.arange(N_HOT) / 26.0
    weight[0] = 1e9
    first_shared = B if private else 0
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols = np.empty(indptr[-1], dtype=np.int64)
    for L in np.unique(lens):
        if L == 0:
            continue
        rows = np.flatnonzero(lens == L)
        m = L - 1 if private else L
        keys = -np.log(rng.random((len(rows), n_sh))) / weight[None, :]
        pick = first_shared + np.argsort(keys, axis=1)[:, :m]
        if private:  # even rows: a column below the shared ones; odd rows: above them
            own = np.where(rows % 2 == 0, rows, B + n_sh + rows)
            pick = np.concatenate([pick, own[:, None]], axis=1)
        cols[indptr[rows][:, None] + np.arange(L)[None, :]] = np.sort(pick, axis=1)
    n = 2 * B + n_sh if private else N_PLAIN
    X = csr_matrix((rng.standard_normal(indptr[-1]), cols.astype(np.int32), indptr), shape=(B, n))
    for L in EDGES:
        assert (lens == L).sum() >= (0 if every_row and L < 2 else B // 20), (L, int((lens == L).sum()))
    y = (rng.random(B) < 0.5).astype(np.int64)
    p = rng.uniform(0.1, 1.0, size=B) ** 0.5
    cnt = np.bincount(X.indices, minlength=n)
    hot = first_shared + np.arange(N_HOT)
    hot_min = int(cnt[hot].min())
    assert np.delete(cnt, hot).max() < hot_min, (hot_min, int(np.delete(cnt, hot).max()))
    if every_row:
        assert cnt[first_shared] == B
    return {"features": X, "labels": y, "pscores": p}, hot_min, hot


@functools.lru_cache(maxsize=None)
def _theta(n, k):
    return gf.perturbed_init(500 + k, n, k)


def _open(rt, log, k, B, hot_mode, want_hot=None, blocks=True, lanes8=True):
    """`lanes8`: a step of B rows on the plan takes the 8-lane kernel (else fm_forward_kernel at the plan's lanes)."""
    dev = gf.DeviceLog(rt, log, k, B, hot_mode)
    try:
        lay = dev.plan.layout()
        assert lay["row_blocks"] == blocks and lay["lanes_per_row"] == gf.CLASS_OF.get(k, (16,))[0], lay
        assert fr.forward_geometry(rt, B, k, True)["block"] == BIG
        form = dev.plan.step_form(B)
        assert form["block"] == BIG and form["lanes8"] == int(lanes8), form
        if lanes8:
            assert form["lanes"] == 8 and form["kind"] == "blocks" and not form["fixed_order"], form
        else:
            assert form["lanes"] == lay["lanes_per_row"], form
            assert form["fixed_order"] == int(hot_mode == -2) and form["kind"].startswith("blocks" if blocks else "records"), form
        if want_hot is not None:
            np.testing.assert_array_equal(np.sort(dev.plan.hot_columns()), want_hot)
    except BaseException:
        dev.close()
        raise
    return dev


# --------------------------------------------------------------------------
# 1. every row's Q row, residual and marks: the bits of the 16-lane map
# --------------------------------------------------------------------------
@pytest.mark.parametrize("size", ["min", "plus_one", "second_trip"])
@pytest.mark.parametrize("k", [32, 20])
def test_every_row_has_the_bits_of_the_16_lane_map(rt, k, size):
    """k = 20: lanes 2 - 7 of a group hold no second pair of factors."""
    B = _sizes(k)[size]
    (log, hot_min, hot), ids = _log(B, True), np.random.default_rng(B).permutation(B).astype(np.int32)
    theta = _theta(log["features"].shape[1], k)
    grads, hots = [], []
    for mode in (hot_min, -2):  # this shape; the 16-lane map at two rows per lane group
        dev = _open(rt, log, k, B, mode, hot if mode == hot_min else None, lanes8=mode == hot_min)
        try:
            assert dev.plan.layout()["longest_row"] == 16
            hots.append(dev.plan.hot_columns())
            grads.append(gf.dense_grad(dev, ids, gf.Params(rt, *theta))[0])
            if mode == hot_min:  # the one-row shape of the same plan, a piece of the batch at a time
                piece = _sizes(k)["min"] - 1
                assert fr.forward_geometry(rt, piece, k, True)["block"] == SMALL
                form = dev.plan.step_form(piece)
                assert (form["block"], form["lanes8"], form["lanes"], form["kind"]) == (SMALL, 0, 16, "blocks"), form
                pieces = [gf.dense_grad(dev, ids[at: at + piece], gf.Params(rt, *theta))[0]
                          for at in range(0, B, piece)][:2]  # (the first two pieces)
        finally:
            dev.close()
    n = log["features"].shape[1]
    (V8, w8, g0_8), (V16, w16, g0_16) = (gf.split_grad(g, n, k) for g in grads)
    assert hots[0].size == N_HOT and hots[1].size > 0
    sparse = np.setdiff1d(np.arange(n), np.union1d(*hots))
    own = np.setdiff1d(sparse, B + np.arange(N_SHARED))
    held = np.flatnonzero(np.diff(log["features"].indptr) > 0)
    assert np.count_nonzero(w8[own]) == len(held) > 0.9 * B  # every row that is not empty, by its own column
    np.testing.assert_array_equal(_bits(V8[sparse]), _bits(V16[sparse]), err_msg="G_V of the sparse class")
    np.testing.assert_array_equal(_bits(w8[sparse]), _bits(w16[sparse]), err_msg="g_w of the sparse class")
    assert _bits(g0_8) == _bits(g0_16), (g0_8, g0_16)
    for at, g in zip(range(0, B, piece), pieces):  # a row's own column: the same bits from the one-row shape
        rows = ids[at: at + piece]
        mine = np.where(rows % 2 == 0, rows, B + N_SHARED + rows)[np.diff(log["features"].indptr)[rows] > 0]
        Vp, wp, _ = gf.split_grad(g, n, k)
        np.testing.assert_array_equal(_bits(V8[mine]), _bits(Vp[mine]), err_msg="G_V against the one-row shape")
        np.testing.assert_array_equal(_bits(w8[mine]), _bits(wp[mine]), err_msg="g_w against the one-row shape")


# --------------------------------------------------------------------------
# 2. the hot columns and the whole gradient against the long-double oracle; one step under both rules
# --------------------------------------------------------------------------
CASES_ORACLE = [(32, "plus_one", False), (32, "second_trip", False), (20, "plus_one", False), (24, "min", True),
                (28, "plus_one", True)]


@functools.lru_cache(maxsize=None)
def _oracle_case(k, size, every_row):
    B = _sizes(k)[size]
    log, hot_min, hot = _log(B, False, every_row)
    theta = _theta(N_PLAIN, k)
    ids = np.random.default_rng(B + k).permutation(B).astype(np.int32)
    return B, log, hot_min, hot, theta, ids, gf.grad_oracle(log, ids, *theta)


@pytest.mark.parametrize("k,size,every_row", CASES_ORACLE, ids=[f"k{k}-{s}{'-col0-in-every-row' if e else ''}"
                                                                  for k, s, e in CASES_ORACLE])
def test_gradient_and_one_step_sgd_and_adagrad(rt, k, size, every_row):
    """Hot ranks 0 - 15 (the tile) and 16 - 23 (the walk); dense columns put one hot column into both rows
    of a 16-lane slice, `every_row` into every row of the batch."""
    B, log, hot_min, hot, theta, ids, oracle = _oracle_case(k, size, every_row)
    dev = _open(rt, log, k, B, hot_min, hot)
    try:
        params = gf.Params(rt, *theta)
        g, _ = gf.dense_grad(dev, ids, params)
        gf.check_dense(g, dev, ids, oracle, dev.plan.hot_columns(), f"k={k} B={B}")
        gf.step(dev, ids, params, STEP_LR)
        for name, ratio in zip(("w0", "w", "V"), gf.step_excess(params.host(), theta, oracle, STEP_LR, B)):
            print(f"SGD {name}: worst |got - (theta - lr g)| / bound = {float(ratio.max()):.3g}")
            assert (ratio <= 1).all(), (name, np.argwhere(ratio > 1)[:5], float(ratio.max()))
        G = ac.acc_init("uniform", N_PLAIN, k, k)
        got_t, got_G = ac.adagrad_step(dev, ids, gf.Params(rt, *theta), gf.Params(rt, *G))
        ac.assert_inside(got_t, got_G, theta, G, oracle, ac.LR, ac.EPS, B, f"AdaGrad k={k} B={B}")
    finally:
        dev.close()


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_row_of_V_reaches_only_the_rows_that_hold_its_column(rt, bad):
    """A sparse column's row of V is not finite: the hot columns of the rows that hold it come out NaN,
    every other hot column is finite and within grad_tol of the oracle over the batch without those rows
    (the rows share wavefronts, 16-lane slices and tile products with rows that are fine)."""
    k = 32
    B, log, _, hot, (w0, w, V), ids, _ = _oracle_case(k, "plus_one", False)
    sparse = N_PLAIN - 1  # (in no row of the log so far)
    holders = np.array([9, 64 + 9, B - 2])  # two rows of the first wavefront's slices, and a row of the last trip
    D = log["features"].toarray()
    D[holders] = 0.0
    D[holders[:, None], np.array([0, 1, 2, sparse])[None, :]] = np.array([0.8, -1.1, 0.5, 1.3])[None, :]
    log = dict(log, features=csr_matrix(D))
    cnt = np.bincount(log["features"].indices, minlength=N_PLAIN)
    hot_min = int(cnt[hot].min())
    assert np.delete(cnt, hot).max() < hot_min
    held, free = hot[:3], hot[3:]
    V_bad, V_fin = V.copy(), V.copy()
    V_bad[sparse, 3] = bad
    V_fin[sparse] = 0.0
    rest = np.setdiff1d(ids, holders).astype(np.int32)
    o_w0, o_w, o_V, (S_0, S_w, S_V) = gf.grad_oracle(log, rest, w0, w, V_fin)
    dev = _open(rt, log, k, B, hot_min, hot)
    try:
        g, _ = gf.dense_grad(dev, ids, gf.Params(rt, w0, w, V_bad))
        G_V, g_w, _ = gf.split_grad(g, N_PLAIN, k)
        assert np.isfinite(G_V[free]).all() and np.isfinite(g_w[free]).all()
        gf.assert_within_scale(G_V[free], o_V[free], S_V[free], gf.grad_tol(B), "G_V of the columns the rows do not hold")
        gf.assert_within_scale(g_w[free], o_w[free], S_w[free], gf.grad_tol(B), "g_w of the columns the rows do not hold")
        assert np.isnan(G_V[held]).all() and np.isnan(g_w[held]).all()
    finally:
        dev.close()


# --------------------------------------------------------------------------
# 3. the plans that keep the 16-lane (or their own) instantiation: the same oracle
# --------------------------------------------------------------------------
CASES_OTHER = [("k30", 30, 0, 16), ("k16", 16, 0, 16), ("fixed-order", 32, -2, 16), ("row-of-20-entries", 32, 0, 20)]


@pytest.mark.parametrize("name,k,mode,longest", CASES_OTHER, ids=[c[0] for c in CASES_OTHER])
def test_plans_outside_the_shape_are_what_they_were(rt, name, k, mode, longest):
    """k = 30 and 16 (no multiple of four in 20 .. 32), fixed-order hot sums, and a plan whose longest row
    does not fit a row block: the dispatch leaves them their instantiations (whose assembly is that of
    the parent commit: profiles/n26/register_counts.txt); their gradients hold against the oracle."""
    B = fr.many_rows_minimum(rt, k, True) + 1
    log, hot_min, hot = _log(B, False, False, longest)
    theta = _theta(N_PLAIN, k)
    ids = np.random.default_rng(B + k).permutation(B).astype(np.int32)
    oracle = gf.grad_oracle(log, ids, *theta)
    dev = _open(rt, log, k, B, hot_min if mode == 0 else mode, hot if mode == 0 else None,
                blocks=longest <= gf.CLASS_OF.get(k, (16,))[0], lanes8=False)
    try:
        assert dev.plan.layout()["longest_row"] == longest
        g, _ = gf.dense_grad(dev, ids, gf.Params(rt, *theta))
        gf.check_dense(g, dev, ids, oracle, dev.plan.hot_columns(), name)
    finally:
        dev.close()


@pytest.mark.parametrize("k", [16, 36])
def test_the_factor_counts_next_to_the_shape_keep_their_kernel(rt, k):
    """k = 16 (8 lanes of fm_forward_kernel: the log's rows of 16 entries stay records) and 36 (32 lanes, row
    blocks), arrival-order hot sums, on the log of the bit tests: no 8-lane kernel (the query alone:
    nothing is launched)."""
    B = fr.many_rows_minimum(rt, k, True)
    log, hot_min, _ = _log(B, True)
    dev = gf.DeviceLog(rt, log, k, B, hot_min)
    try:
        lay, form = dev.plan.layout(), dev.plan.step_form(B)
        assert lay["row_blocks"] == (k == 36) and form["block"] == BIG and form["lanes8"] == 0, (lay, form)
        assert form["lanes"] == lay["lanes_per_row"] == (8 if k == 16 else 32), (lay, form)
        assert form["kind"] == ("blocks" if k == 36 else "records") and not form["fixed_order"], (lay, form)
    finally:
        dev.close()
