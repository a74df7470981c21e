"""The hot tile of the FM forward: at 16 lanes x 2 factors per row (k = 18 ... 32 even, training
records, arrival-order hot sums) the 16 most frequent hot columns' err * x * q are summed by
v_mfma_f64_16x16x4 and flushed into the workgroup's LDS sums once per round; the other hot entries
are walked, compacted to the front of the round.  Needs an MI355X: ``pytest -m gpu``.

Every case builds a log with ``grad_forms_common._bounded_log`` (H dense columns: column c is in
every row longer than c), overwrites a few batch positions with the row forms named below, sets
``hot_min_count`` to the count of the rarest dense column and ASSERTS that the plan's hot class is
exactly those H columns and that the step takes the workgroup shape the case is meant for.  The
dense gradient is held to the long-double oracle element by element, |got - want| <= grad_tol(B) * S
(grad_forms_common: derived, not measured), every column of G_V and g_w and g_w0; then one in-place
step against theta - lr * g within ``step_bound``.

H: 1, 15 (a tile partly filled), 16 (exactly full), 17, 33 (ranks spilling to the walk; rows of up
to 40 entries: plain records, several rounds, the tile flushed per round), and 24 with the dense
columns of every other row shifted by 8 (rows of at most 16 entries -- the padded row blocks -- that
hold tile and walked entries side by side).  k: 32, 30, 18 (lanes 9 - 15 of a group hold no factor).
B: 5 and 300 (one-row shape; at 5 three lane groups of a wavefront are idle), 16 384 + 3 (many-rows
shape, a last trip of invalid rows).  Row forms, at fixed batch positions (ids are the identity):
positions 0 - 3 and 64 - 67 -- the two rows of each lane group of the first wavefront of either
shape -- hold only the first min(H, 16) columns, so that wavefront walks nothing and positions
g, g + 64 hold the same ranks; position 4 has x = 0 and x < 0 on dense columns; position 5 (B > 5)
holds no hot column at all; empty rows, rows of 1 and of 16 entries come with the random part (asserted)."""
import functools

import numpy as np
import pytest
from scipy.sparse import csr_matrix

import forward_rows_common as fr
import grad_forms_common as gf

pytestmark = pytest.mark.gpu

BIG = 16384 + 3
STEP_LR = 2.0 ** -3
TILE = 16


@pytest.fixture(scope="module")
def rt():
    from relevance_factorizationmachine_amd import runtime
    return runtime.Runtime.get()


def _replace_rows(log, rows):
    """`log` with the rows {position: (columns, values)} written over (explicit zeros are kept)."""
    X = log["features"]
    indptr, cols, vals = [0], [], []
    for r in range(X.shape[0]):
        if r in rows:
            c, v = rows[r]
        else:
            c, v = X.indices[X.indptr[r]: X.indptr[r + 1]], X.data[X.indptr[r]: X.indptr[r + 1]]
        cols.extend(int(x) for x in c)
        vals.extend(float(x) for x in v)
        indptr.append(len(cols))
    out = dict(log)
    out["features"] = csr_matrix((np.array(vals, dtype=np.float64), np.array(cols, dtype=np.int32),
                                  np.array(indptr, dtype=np.int64)), shape=X.shape)
    return out


@functools.lru_cache(maxsize=None)
def _case(H, k, B, shifted=False):
    """Log, hot_min_count, parameters, ids and the oracle of a case: computed once, never modified."""
    rng = np.random.default_rng(1000 * H + 10 * k + B % 97 + shifted)
    max_len = 16 if H <= TILE or shifted else 40
    n_cols = 64 if B > 1000 else 96
    dense = 16 if shifted else H
    log = gf._bounded_log(rng, B, n_cols, max_len, dense)
    X = log["features"]
    if shifted:  # every other row: dense column c -> c + 8 (columns 8 - 23; H = 24 hot columns)
        assert H == 24
        idx = X.indices.copy()
        for r in range(1, B, 2):
            seg = idx[X.indptr[r]: X.indptr[r + 1]]
            # (the sparse columns of the row move behind the shifted dense ones)
            seg[:] = np.sort(np.where(seg < dense, seg + 8, np.where(seg < dense + 8, seg + 40, seg)))
            assert len(np.unique(seg)) == len(seg)
        X = csr_matrix((X.data, idx, X.indptr), shape=X.shape)
        log = dict(log, features=X)
    lens = np.diff(X.indptr)
    assert B < 100 or ((lens == 0).any() and (lens == 1).any() and (lens == 16).any())
    first = list(range(min(H, TILE)))
    rows = {}
    if B > 67 and not shifted:
        for pos in (0, 1, 2, 3, 64, 65, 66, 67):
            rows[pos] = (first, rng.standard_normal(len(first)))
    zrow = first[:3]
    rows[4] = (zrow, [0.0, -1.5, 0.7][: len(zrow)])  # x = 0 and x < 0 on tile entries
    if B > 5:
        rows[5] = ([H + 1, H + 3], [0.9, -0.4])  # no hot column
    log = _replace_rows(log, rows)
    X = log["features"]
    cnt = np.bincount(X.indices, minlength=n_cols)
    hot_min = int(cnt[:H].min())
    assert hot_min >= 1 and cnt[H:].max() < hot_min, (cnt[:H].min(), cnt[H:].max())
    w0, w, V = gf.perturbed_init(H + k, n_cols, k)
    ids = np.arange(B, dtype=np.int32)
    return log, hot_min, (w0, w, V), ids, gf.grad_oracle(log, ids, w0, w, V)


def _open(rt, log, k, B, hot_min, H):
    dev = gf.DeviceLog(rt, log, k, B, hot_min)
    try:
        assert dev.plan.layout()["lanes_per_row"] == 16
        assert dev.plan.info()["hot_columns"] == H, dev.plan.info()
        np.testing.assert_array_equal(np.sort(dev.plan.hot_columns()), np.arange(H))
        assert fr.forward_geometry(rt, B, k, True)["block"] == (1024 if B == BIG else 256)
    except BaseException:
        dev.close()
        raise
    return dev


def _check(rt, H, k, B, shifted=False):
    log, hot_min, theta, ids, oracle = _case(H, k, B, shifted)
    dev = _open(rt, log, k, B, hot_min, H)
    try:
        longest = dev.plan.layout()["longest_row"]
        assert (longest <= 16) == (H <= TILE or shifted), longest
        params = gf.Params(rt, *theta)
        g, _ = gf.dense_grad(dev, ids, params)
        gf.check_dense(g, dev, ids, oracle, dev.plan.hot_columns(), f"H={H} k={k} B={B}")
        gf.step(dev, ids, params, STEP_LR)
        got = params.host()
        for name, ratio in zip(("w0", "w", "V"), gf.step_excess(got, theta, oracle, STEP_LR, B)):
            print(f"{name}: worst |got - (theta - lr g)| / bound = {float(ratio.max()):.3g}")
            assert (ratio <= 1).all(), (name, np.argwhere(ratio > 1)[:5], float(ratio.max()))
    finally:
        dev.close()


# one round (rows of at most 16 entries), the tile partly filled / exactly full
CASES_ONE = ([(H, k, 300) for H in (1, 15, 16) for k in (32, 30, 18)] +
             [(1, 32, 5), (16, 18, 5), (15, 30, 5), (16, 32, 5)] +
             [(16, 32, BIG), (15, 30, BIG), (1, 18, BIG), (16, 18, BIG)])
# several rounds (rows of up to 40 entries), ranks past the tile on the walk
CASES_MANY = [(17, 32, 300), (33, 32, 300), (17, 18, 300), (33, 30, 300), (17, 30, 5), (33, 32, 5),
              (33, 32, BIG), (17, 18, BIG)]
# one round, tile and walked entries in one row
CASES_MIXED = [(24, 32, 300), (24, 18, 300), (24, 32, BIG), (24, 18, BIG)]


@pytest.mark.parametrize("H,k,B", CASES_ONE, ids=[f"H{H}-k{k}-B{B}" for H, k, B in CASES_ONE])
def test_tile_one_round(rt, H, k, B):
    _check(rt, H, k, B)


@pytest.mark.parametrize("H,k,B", CASES_MANY, ids=[f"H{H}-k{k}-B{B}" for H, k, B in CASES_MANY])
def test_tile_and_walk_over_several_rounds(rt, H, k, B):
    _check(rt, H, k, B)


@pytest.mark.parametrize("H,k,B", CASES_MIXED, ids=[f"H{H}-k{k}-B{B}" for H, k, B in CASES_MIXED])
def test_tile_and_walk_in_one_round(rt, H, k, B):
    _check(rt, H, k, B, shifted=True)


@pytest.mark.parametrize("bad", [float("nan"), float("inf")], ids=["nan", "inf"])
@pytest.mark.parametrize("B", [300, BIG])
def test_a_non_finite_row_of_V_stays_in_the_columns_of_its_rows(rt, B, bad):
    """Batch position 9 (a wavefront it shares with rows that are fine) holds hot columns 0 - 2 and a
    sparse column whose row of V is not finite: the hot columns it holds come out NaN, every other
    hot column is finite and within grad_tol of the oracle over the batch without that row."""
    H, k = 16, 32
    log, hot_min, (w0, w, V), ids, _ = _case(H, k, B)
    sparse = H + 7
    log = _replace_rows(log, {9: ([0, 1, 2, sparse], [0.8, -1.1, 0.5, 1.3])})
    X = log["features"]
    cnt = np.bincount(X.indices, minlength=X.shape[1])
    hot_min = int(cnt[:H].min())
    assert cnt[H:].max() < hot_min
    holders = np.unique(X[:, sparse].nonzero()[0])
    rest = np.setdiff1d(ids, holders).astype(np.int32)
    assert 9 in holders and len(holders) < B // 4
    held = np.unique(X[holders].indices)
    free = np.setdiff1d(np.arange(H), held)
    assert len(free) >= 8 and {0, 1, 2} <= set(held.tolist())
    V_bad = V.copy()
    V_bad[sparse, 3] = bad
    V_fin = V.copy()
    V_fin[sparse] = 0.0  # (no row of `rest` holds the column: its row of V does not enter)
    oracle = gf.grad_oracle(log, rest, w0, w, V_fin)
    dev = _open(rt, log, k, B, hot_min, H)
    try:
        g, _ = gf.dense_grad(dev, ids, gf.Params(rt, w0, w, V_bad))
        G_V, g_w, _ = gf.split_grad(g, dev.n, k)
        o_w0, o_w, o_V, (S_0, S_w, S_V) = oracle
        tol = gf.grad_tol(B)
        assert np.isfinite(G_V[free]).all() and np.isfinite(g_w[free]).all()
        gf.assert_within_scale(G_V[free], o_V[free], S_V[free], tol, "G_V of the hot columns the row does not hold")
        gf.assert_within_scale(g_w[free], o_w[free], S_w[free], tol, "g_w of the hot columns the row does not hold")
        hot_held = np.intersect1d(held, np.arange(H))
        assert np.isnan(G_V[hot_held]).all() and np.isnan(g_w[hot_held]).all()
    finally:
        dev.close()
