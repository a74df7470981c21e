"""The long-double gradient oracle of grad_forms_common.py, checked on the host before any device
result is held to it: against cpu_ref.fm_gradients and against central finite differences of the
loss whose gradient it states."""
import numpy as np
import pytest
from scipy.sparse import csr_matrix

import grad_forms_common as gf
from oracle import cpu_ref

LD = np.longdouble


def _tiny_log(seed, n_rows, n_cols, k):
    """A dense-ish tiny log with an empty row, an explicitly stored zero and propensities below 1."""
    rng = np.random.default_rng(seed)
    D = rng.standard_normal((n_rows, n_cols)) * (rng.random((n_rows, n_cols)) < 0.5)
    D[1, :] = 0.0  # an empty row
    D[0, 0] = 1.5
    X = csr_matrix(D)
    X.data[0] = 0.0  # an explicit zero (row 0, column 0), kept in the structure
    D[0, 0] = 0.0
    assert X.nnz == np.count_nonzero(D) + 1 and X[1].nnz == 0
    y = (rng.random(n_rows) < 0.5).astype(np.float64)
    y[0] = 1.0
    p = rng.uniform(0.2, 0.9, size=n_rows)
    w0, w, V = gf.perturbed_init(seed, n_cols, k)
    return X, D, y, p, w0, w, V


def _loss_ld(D, y, p, w0, w, V):
    """-sum_t [(y/p) log s + (1 - y/p) log(1 - s)], no eps, in long double."""
    z, _ = gf.fm_logit_ld(D.astype(LD), LD(w0), w.astype(LD), V.astype(LD))
    r = y.astype(LD) / p.astype(LD)
    # log s = -log(1 + e^-z), log(1 - s) = -log(1 + e^z): no cancellation at a saturated logit
    return (r * np.logaddexp(LD(0), -z) + (1 - r) * np.logaddexp(LD(0), z)).sum()


CASES = [(11, 12, 9, 1), (12, 7, 5, 3), (13, 10, 8, 4)]


@pytest.mark.parametrize("seed,n_rows,n_cols,k", CASES)
def test_oracle_matches_cpu_ref(seed, n_rows, n_cols, k):
    X, D, y, p, w0, w, V = _tiny_log(seed, n_rows, n_cols, k)
    g_w0, g_w, G_V, (S_0, S_w, S_V) = gf.fm_gradients_ld(X, y, p, w0, w, V)
    assert G_V.dtype == LD and G_V.shape == (n_cols, k) and g_w.shape == (n_cols,)
    _, r_w0, r_w, r_V = cpu_ref.fm_gradients(X, y, p, w0, w, V)
    # float64 against long double: the bound every device gradient is held to
    gf.assert_within_scale(r_V, G_V, S_V, gf.GRAD_TOL, "G_V")
    gf.assert_within_scale(r_w, g_w, S_w, gf.GRAD_TOL, "g_w")
    gf.assert_within_scale(r_w0, g_w0, S_0, gf.GRAD_TOL, "g_w0")
    # the scales dominate the values they bound; a column nobody holds has scale and gradient 0
    assert (np.abs(G_V) <= S_V * (1 + 1e-15)).all() and (np.abs(g_w) <= S_w * (1 + 1e-15)).all()
    assert abs(g_w0) <= S_0
    empty = np.flatnonzero(np.count_nonzero(D, axis=0) == 0)
    assert not S_V[empty].any() and not G_V[empty].any()
    # the same from the dense array
    d_w0, d_w, d_V, _ = gf.fm_gradients_ld(D, y, p, w0, w, V)
    assert d_w0 == g_w0 and (d_w == g_w).all() and (d_V == G_V).all()


@pytest.mark.parametrize("seed,n_rows,n_cols,k", CASES)
def test_oracle_matches_central_differences(seed, n_rows, n_cols, k):
    """Central differences at h = 1e-6 agree to 1e-7 * max(1, |g|): their truncation order."""
    X, D, y, p, w0, w, V = _tiny_log(seed, n_rows, n_cols, k)
    g_w0, g_w, G_V, _ = gf.fm_gradients_ld(X, y, p, w0, w, V)
    h = LD(1e-6)
    w0, w, V = LD(w0[0]), w.astype(LD), V.astype(LD)

    def diff(f):
        return (f(h) - f(-h)) / (2 * h)

    def close(fd, g):
        return abs(fd - g) <= 1e-7 * max(1.0, abs(g))

    assert close(diff(lambda d: _loss_ld(D, y, p, w0 + d, w, V)), g_w0)
    for c in range(n_cols):
        def at_w(d):
            w2 = w.copy()
            w2[c] += d
            return _loss_ld(D, y, p, w0, w2, V)
        assert close(diff(at_w), g_w[c]), ("w", c)
        for f in range(k):
            def at_v(d):
                V2 = V.copy()
                V2[c, f] += d
                return _loss_ld(D, y, p, w0, w, V2)
            assert close(diff(at_v), G_V[c, f]), ("V", c, f)


def test_within_scale_is_elementwise():
    """A rare column's error does not hide under a dense column's magnitude."""
    want, scale = np.array([1e6, 1e-3]).astype(LD), np.array([1e6, 1e-3]).astype(LD)
    gf.assert_within_scale(np.array([1e6 + 5e-6, 1e-3]), want, scale, 1e-11, "ok")
    with pytest.raises(AssertionError):
        gf.assert_within_scale(np.array([1e6, 1e-3 + 1e-9]), want, scale, 1e-11, "rare column")
    with pytest.raises(AssertionError):
        gf.assert_within_scale(np.array([1e6, np.nan]), want, scale, 1e-11, "NaN")
    assert gf.grad_tol(1_500) == gf.GRAD_TOL and gf.grad_tol(80_000) == 2 * gf.GRAD_TOL


def _step_f64(log, theta, lr, order, drop=None):
    """One in-place step on the whole log in float64, every column's sums (m = sum coef * q_t,
    sum coef, sum coef * x) added one term at a time in the row order `order`; `drop` = (column,
    rows): that column's sums miss those rows' terms."""
    w0, w, V = theta
    X = log["features"].toarray()
    q = X @ V
    z = w0[0] + X @ w + ((q * q).sum(axis=1) - (X * X) @ (V * V).sum(axis=1)) / 2
    e = log["labels"] / log["pscores"] - 1 / (1 + np.exp(-np.clip(z, -cpu_ref.LOGIT_CLIP, cpu_ref.LOGIT_CLIP)))
    new_w, new_V = w.copy(), V.copy()
    for c in range(X.shape[1]):
        rows = [t for t in order if X[t, c] != 0 and not (drop and drop[0] == c and t in drop[1])]
        coef = e[rows] * X[rows, c]
        m = np.cumsum(coef[:, None] * q[rows], axis=0)[-1] if rows else np.zeros(V.shape[1])
        gw, d = (np.cumsum(coef)[-1], np.cumsum(coef * X[rows, c])[-1]) if rows else (0.0, 0.0)
        new_V[c] = V[c] + lr * (m - d * V[c])
        new_w[c] = w[c] + lr * gw
    return np.array([w0[0] + lr * np.cumsum(e[order])[-1]]), new_w, new_V


def test_step_bound_on_the_smallest_split_geometry():
    """grad_forms_common.step_bound on the smallest case of test_split_columns_in_gradient_mode (64
    lanes per row, short form: 256 slots to a workgroup, column 0 in two partial rows): a float64
    step with every sum's terms in shuffled order stays below HALF the bound on every element; a
    step that loses one partial row of the split column is outside it on that column's V row and
    w, and nowhere else."""
    k = min(k for k, _ in gf.CASES_B if gf.CLASS_OF[k][0] == 64)
    bc = gf.full_batch_workgroup_slots(k)
    assert bc == min(gf.full_batch_workgroup_slots(k2) for k2, _ in gf.CASES_B)
    n_rows, lr = bc + 37, 2.0 ** -3
    log, theta, full, _ = gf.split_case(k, n_rows, 60, 1, 7 * k + len("short"))
    oracle = gf.grad_oracle(log, full, *theta)
    order = [int(t) for t in np.random.default_rng(5).permutation(n_rows)]
    for ratio in gf.step_excess(_step_f64(log, theta, lr, order), theta, oracle, lr, n_rows):
        assert (ratio < 0.5).all(), float(ratio.max())
    # column 0's entries in row (= slot) order: a workgroup's slots to a partial row
    holders = np.flatnonzero(log["features"].toarray()[:, 0])
    assert bc < len(holders) <= 2 * bc
    lost = _step_f64(log, theta, lr, order, drop=(0, set(holders[bc:].tolist())))
    r_w0, r_w, r_V = gf.step_excess(lost, theta, oracle, lr, n_rows)
    assert (r_V[0] > 1).all() and r_w[0] > 1
    assert (r_V[1:] <= 1).all() and (r_w[1:] <= 1).all() and (r_w0 <= 1).all()
