"""Shared by the tests of the FM gradient forms (test_grad_oracle_host.py, test_gpu_grad_forms.py),
by the row-by-row tests of the FM forward (forward_rows_common.py, test_gpu_forward_rows.py) and
by test_gpu_parity.py: the table of kernel classes, the small random logs, the long-double
statement of the batch-SUM gradients with the magnitude every sum adds up, thin wrappers of the
raw ABI calls (rfm_fm_grad, rfm_fm_grad_rows, ...) that fill their outputs with NaN first and keep
guard records behind them, and the comparisons of a plan's dense gradient and record list.
Importing this module touches neither the GPU nor the package under test.

Tolerance of a device gradient against ``fm_gradients_ld``: element-wise
``|got - want| <= GRAD_TOL * S`` with S the sum of the absolute values of the terms of that
element's sum.  A float64 sum of n terms in any order is off by at most (n-1) * 2^-53 * sum|terms|,
i.e. 4.4e-12 * S at 40 000 rows, the largest batch used; the residuals and row sums carry a few
row lengths of 2^-53 relative on top.  1e-11 covers both; it is derived, not measured.

Tolerance of a parameter after one in-place step of learning rate lr against theta - lr * g, g the
oracle's gradient: element-wise ``lr * GRAD_TOL * S + 2^-52 * (|theta| + lr * S)`` (`step_bound`).
The device forms theta + lr * (-g_dev) from the same sums as its gradient, so |g_dev - g| <=
GRAD_TOL * S carries over scaled by lr: the first term.  The product lr * g_dev is exact for a
power of two lr, else within 2^-53 * lr * |g_dev| <= 2^-53 * lr * S; the final addition rounds
its result, of magnitude at most |theta| + lr * S, by 2^-53 relative (whether or not the product
was fused into it); rounding the long-double reference to compare adds less.  Together under
2^-52 * (|theta| + lr * S): the second term."""
import numpy as np
from scipy.sparse import csr_matrix, random as sprandom

from oracle import cpu_ref

GRAD_TOL = 1e-11
GRAD_TOL_ROWS = 40_000  # batch rows GRAD_TOL is derived for
GUARD = 8               # records kept behind a record list's capacity
LD = np.longdouble


# --------------------------------------------------------------------------
# logs
# --------------------------------------------------------------------------
def _random_log(rng, n_rows, n_cols, density, dense_cols=0):
    X = sprandom(n_rows, n_cols, density=density, format="csr", random_state=rng,
                 data_rvs=lambda s: rng.standard_normal(s)).tolil()
    for c in range(dense_cols):  # a few columns present in every row (long column lists)
        X[:, c] = rng.standard_normal(n_rows)[:, None]
    X = X.tocsr()
    X.sort_indices()
    y = (rng.random(n_rows) < 0.5).astype(np.int64)
    p = rng.uniform(0.1, 1.0, size=n_rows) ** 0.5
    return {"features": X, "labels": y, "pscores": p}


def _bounded_log(rng, n_rows, n_cols, max_len, dense_cols):
    """Rows of 0..max_len entries (a few empty), `dense_cols` columns in (almost) every row."""
    lens = rng.integers(0, max_len + 1, size=n_rows)
    lens[rng.integers(0, n_rows, size=5)] = 0
    lens[rng.integers(0, n_rows, size=5)] = max_len
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols = np.empty(indptr[-1], dtype=np.int32)
    for r in range(n_rows):
        m = lens[r]
        if m:
            d = min(dense_cols, m)
            rest = rng.choice(np.arange(dense_cols, n_cols), size=m - d, replace=False) if m > d else []
            cols[indptr[r]: indptr[r + 1]] = np.sort(np.concatenate([np.arange(d), rest]).astype(np.int32))
    X = csr_matrix((rng.standard_normal(indptr[-1]), cols, indptr), shape=(n_rows, n_cols))
    y = (rng.random(n_rows) < 0.5).astype(np.int64)
    p = rng.uniform(0.1, 1.0, size=n_rows) ** 0.5
    return {"features": X, "labels": y, "pscores": p}


def split_case(k, n_rows, n_cols, dense_cols, seed):
    """A log whose first `dense_cols` columns are in every row but two (a split column once the
    rows outnumber a workgroup's slots), parameters, the full batch in shuffled order, a shard."""
    rng = np.random.default_rng(seed)
    log = _random_log(rng, n_rows, n_cols, 0.05, dense_cols)
    D = log["features"].toarray()
    D[[3, n_rows // 2], :] = 0.0  # empty rows (the dense columns miss them)
    log["features"] = csr_matrix(D)
    w0, w, V = perturbed_init(seed, n_cols, k)
    full = rng.permutation(n_rows).astype(np.int32)
    shard = np.array([n_rows - 1, 3, 0, n_rows // 3, 17], dtype=np.int32)
    return log, (w0, w, V), full, shard


def perturbed_init(seed, n, k):
    """cpu_ref.fm_init with w0 and every w[c] moved off zero."""
    w0, w, V = cpu_ref.fm_init(seed, n, k)
    rng = np.random.default_rng(seed + 1)
    w0 = np.array([0.37])
    w = w + np.where(rng.random(n) < 0.5, -1.0, 1.0) * rng.uniform(0.05, 0.3, size=n)
    return w0, w, V


# --------------------------------------------------------------------------
# the oracle
# --------------------------------------------------------------------------
def fm_logit_ld(X, w0, w, V):
    """Logit of dense long-double X [m, n] (src/fm.py:124-131), and q = X V."""
    q = X @ V
    pair = (q * q).sum(axis=1) - (X * X) @ (V * V).sum(axis=1)
    return w0 + X @ w + pair / 2, q


def fm_gradients_ld(Xb, yb, pb, w0, w, V):
    """Closed form of cpu_ref.fm_gradients (batch-SUM gradients, no 1/|B|) in np.longdouble on
    dense arrays.  Returns ``(g_w0, g_w, G_V, (S_0, S_w, S_V))``, the last the sum of the absolute
    values of the terms each sum adds:
        S_V[c, f] = sum_t |e_t| (|x_tc| |q_tf| + x_tc^2 |V_cf|),  S_w[c] = sum_t |e_t x_tc|,
        S_0 = sum_t |e_t|."""
    X = np.asarray(Xb.toarray() if hasattr(Xb, "toarray") else Xb).astype(LD)
    w0 = LD(np.asarray(w0, dtype=np.float64).reshape(-1)[0])
    w, V = np.asarray(w).astype(LD), np.asarray(V).astype(LD)
    z, q = fm_logit_ld(X, w0, w, V)
    z = np.clip(z, -LD(cpu_ref.LOGIT_CLIP), LD(cpu_ref.LOGIT_CLIP))
    e = np.asarray(yb).astype(LD) / np.asarray(pb).astype(LD) - 1 / (1 + np.exp(-z))
    Xsq, ae, aX = X * X, np.abs(e), np.abs(X)
    g_w0 = -e.sum()
    g_w = -(X.T @ e)
    G_V = -(X.T @ (e[:, None] * q)) + (Xsq.T @ e)[:, None] * V
    S_0 = ae.sum()
    S_w = aX.T @ ae
    S_V = aX.T @ (ae[:, None] * np.abs(q)) + (Xsq.T @ ae)[:, None] * np.abs(V)
    return g_w0, g_w, G_V, (S_0, S_w, S_V)


def grad_tol(n_rows):
    """GRAD_TOL, scaled with the rows of the batch where they exceed what it is derived for."""
    return GRAD_TOL * max(1.0, n_rows / GRAD_TOL_ROWS)


def step_bound(theta, scale, lr, n_rows):
    """Element-wise bound of a parameter after one in-place step against theta - lr * g (see the
    module's docstring); `scale` = that element's S."""
    return lr * LD(grad_tol(n_rows)) * scale + LD(2.0) ** -52 * (np.abs(theta) + lr * scale)


def step_excess(got, theta, oracle, lr, n_rows):
    """``|got - (theta - lr * g)| / step_bound`` element by element, for (w0, w, V) in that order:
    a step holds where every ratio is <= 1.  got, theta: (w0 [1], w [n], V [n, k])."""
    g_w0, g_w, G_V, (S_0, S_w, S_V) = oracle
    out = []
    for x, t, g, S in zip(got, theta, (g_w0, g_w, G_V), (S_0, S_w, S_V)):
        x, t = np.asarray(x, dtype=np.float64), np.asarray(t).astype(LD)
        g, S = np.broadcast_to(g, t.shape), np.broadcast_to(S, t.shape)
        assert x.shape == t.shape and not np.isnan(x).any()
        err, bound = np.abs(x.astype(LD) - (t - lr * g)), step_bound(t, S, lr, n_rows)
        out.append(np.where(bound > 0, err / np.where(bound > 0, bound, 1), np.where(err > 0, np.inf, 0)))
    return out


def assert_within_scale(got, want, scale, tol, what):
    """Element-wise ``|got - want| <= tol * scale`` (NaN anywhere counts as outside)."""
    got = np.asarray(got, dtype=np.float64)
    want, scale = np.asarray(want), np.asarray(scale)
    assert got.shape == want.shape == scale.shape, (what, got.shape, want.shape, scale.shape)
    bad = ~(np.abs(got.astype(LD) - want) <= LD(tol) * scale)
    if bad.any():
        ratio = np.where(scale > 0, np.abs(got.astype(LD) - want) / np.where(scale > 0, scale, 1), np.inf)
        i = np.unravel_index(int(np.argmax(np.where(bad, ratio, -1))), got.shape) if got.ndim else ()
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} elements outside {tol} * S; worst at "
                             f"{i}: got {got[i]!r}, want {float(want[i])!r}, S {float(scale[i])!r}")


def split_grad(g, n, k):
    """[G_V (n*k) | g_w (n) | g_w0] -> (G_V [n, k], g_w [n], g_w0)."""
    return g[: n * k].reshape(n, k), g[n * k: n * k + n], g[n * k + n]


# --------------------------------------------------------------------------
# the raw ABI calls
# --------------------------------------------------------------------------
class Params:
    """w0, w, V on the device (plain torch tensors: what the ABI takes)."""

    def __init__(self, rt, w0, w, V):
        self.rt = rt
        self.w0, self.w, self.V = rt.upload(w0, dtype=np.float64), rt.upload(w, dtype=np.float64), rt.upload(
            V, dtype=np.float64)
        self.n, self.k = V.shape

    def ptrs(self):
        return self.w0.data_ptr(), self.w.data_ptr(), self.V.data_ptr()

    def host(self):
        self.rt.sync()
        return self.w0.cpu().numpy(), self.w.cpu().numpy(), self.V.cpu().numpy()


class DeviceLog:
    """A log on the device with one plan: ``max_batch`` rows at most per step."""

    def __init__(self, rt, log, k, max_batch, hot=0):
        from relevance_factorizationmachine_amd.fm import FmPlan
        from relevance_factorizationmachine_amd.runtime import DeviceCSR

        self.rt, self.k = rt, k
        self.X = log["features"]
        self.n_rows, self.n = self.X.shape
        self.csr = DeviceCSR(rt, self.X)
        self.y = rt.upload(log["labels"], dtype=np.float64)
        self.p = rt.upload(log["pscores"], dtype=np.float64)
        self.plan = FmPlan(rt, self.csr, self.y, self.p, k, max_batch, hot)

    def log_ptrs(self):
        c = self.csr
        return c.indptr.data_ptr(), c.indices.data_ptr(), c.values.data_ptr(), self.y.data_ptr(), self.p.data_ptr()

    def geometry(self):
        """Plan geometry from the public calls: lane groups of a workgroup, slots of a workgroup."""
        info = self.plan.info()
        gpb = 256 // self.plan.layout()["lanes_per_row"]
        return {"GPB": gpb, "BC": info["slots"] // (info["tasks"] // gpb)}

    def partial_rows(self, col):
        """Partial rows of a column of the sparse class: ceil(len / BC)."""
        length = int(self.X.getnnz(axis=0)[col])
        return -(-length // self.geometry()["BC"])

    def close(self):
        self.plan.close()


def step(dev, ids, params, lr):
    from relevance_factorizationmachine_amd import _lib
    d_ids = dev.rt.upload(np.asarray(ids, dtype=np.int32))
    _lib.check(dev.rt.lib.rfm_fm_step(dev.rt.ctx, dev.plan.handle, *dev.log_ptrs(), d_ids.data_ptr(), len(ids),
                                      *params.ptrs(), lr))
    dev.rt.sync()


def dense_grad(dev, ids, params):
    """rfm_fm_grad into a buffer filled with NaN beforehand -> host array [n*(k+1)+1]."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    rt = dev.rt
    d_ids = rt.upload(np.asarray(ids, dtype=np.int32))
    grad = torch.full((dev.n * (dev.k + 1) + 1,), float("nan"), dtype=torch.float64, device=rt.torch_device)
    _lib.check(rt.lib.rfm_fm_grad(rt.ctx, dev.plan.handle, *dev.log_ptrs(), d_ids.data_ptr(), len(ids),
                                  *params.ptrs(), grad.data_ptr()))
    rt.sync()
    return grad.cpu().numpy(), grad


class Records:
    """What rfm_fm_grad_rows left: ``count`` (the true number), ``rec`` = all cap + GUARD records of
    the NaN-filled buffer, ``gw0``, ``bounds`` (or None), and the device tensors of the call."""

    def filled(self):
        return self.rec[: min(self.count, self.cap)]

    def assert_rest_untouched(self):
        rest = self.rec[min(self.count, self.cap):]
        assert np.isnan(rest).all(), "a record past the count (or a guard record) was written"


def grad_rows(dev, ids, params, cap, ranges=None):
    """rfm_fm_grad_rows with room for ``cap`` records, in a NaN-filled buffer of cap + GUARD."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    rt, k = dev.rt, dev.k
    out = Records()
    out.cap = cap
    out.d_rows = torch.full((cap + GUARD, k + 2), float("nan"), dtype=torch.float64, device=rt.torch_device)
    out.d_n = torch.full((1,), -7, dtype=torch.int32, device=rt.torch_device)
    out.d_gw0 = torch.full((1,), float("nan"), dtype=torch.float64, device=rt.torch_device)
    nr = 0 if ranges is None else len(ranges)
    d_lo = rt.upload(np.asarray(ranges, dtype=np.int32)) if nr else None
    d_bounds = torch.full((nr + 1,), -7, dtype=torch.int32, device=rt.torch_device) if nr else None
    d_ids = rt.upload(np.asarray(ids, dtype=np.int32)) if len(ids) else None
    _lib.check(rt.lib.rfm_fm_grad_rows(
        rt.ctx, dev.plan.handle, d_ids.data_ptr() if d_ids is not None else None, len(ids), *params.ptrs(),
        out.d_rows.data_ptr(), cap, out.d_n.data_ptr(), out.d_gw0.data_ptr(),
        d_lo.data_ptr() if nr else None, nr, d_bounds.data_ptr() if nr else None))
    rt.sync()
    out.count = int(out.d_n.cpu()[0])
    out.rec = out.d_rows.cpu().numpy()
    out.gw0 = float(out.d_gw0.cpu()[0])
    out.bounds = d_bounds.cpu().numpy() if nr else None
    return out


# --------------------------------------------------------------------------
# the kernel classes
# --------------------------------------------------------------------------
# (lanes per row, factors per lane and chunk, chunks per lane) of every factor count used by the tests:
# one k per class that the dispatch on the factor count can return
CLASS_OF = {
    8: (4, 2, 1), 16: (8, 2, 1), 32: (16, 2, 1), 64: (32, 2, 1), 128: (64, 2, 1), 200: (64, 2, 2),
    300: (64, 2, 3), 400: (64, 2, 4), 1024: (64, 2, 8),
    1: (4, 1, 1), 3: (4, 1, 1), 7: (8, 1, 1), 13: (16, 1, 1), 31: (32, 1, 1), 63: (64, 1, 1), 65: (64, 1, 2),
    191: (64, 1, 3), 255: (64, 1, 4), 511: (64, 1, 8), 513: (64, 1, 16),
    33: (64, 1, 1),
}


def full_batch_workgroup_slots(k):
    """Slots of a workgroup of the gradient launch on a plan whose batch is the whole log: every
    slot is then expected marked, a task is one 64-slot word, and a workgroup has one task per
    lane group of its 256 threads.  (test_gpu_grad_forms.py holds the plans to it.)"""
    return 256 // CLASS_OF[k][0] * 64


def class_id(k):
    lpr, vec, nc = CLASS_OF[k]
    return f"lpr{lpr}-vec{vec}-nc{nc}-k{k}"


def chunked(k):
    return CLASS_OF[k][2] > 1


# split columns in gradient mode (test_gpu_grad_forms.py): (factor count, hot mode)
CASES_B = [(8, -1), (33, -1), (128, -1), (65, 0), (300, 0)]


def fixed_order(k, hot):
    return hot in (-1, -2) or chunked(k)


# --------------------------------------------------------------------------
# the comparisons of a plan's gradient forms (test_gpu_grad_forms.py, test_gpu_forward_rows.py)
# --------------------------------------------------------------------------
def check_dense(g, dev, ids, oracle, hot_cols, what):
    """A dense gradient against the oracle; exact zeros where no row of the batch holds the column."""
    n, k = dev.n, dev.k
    assert not np.isnan(g).any(), f"{what}: an element of d_grad was not written"
    G_V, g_w, g_w0 = split_grad(g, n, k)
    o_w0, o_w, o_V, (S_0, S_w, S_V) = oracle
    tol = grad_tol(len(ids))
    assert_within_scale(G_V, o_V, S_V, tol, f"{what} G_V")
    assert_within_scale(g_w, o_w, S_w, tol, f"{what} g_w")
    assert_within_scale(g_w0, o_w0, S_0, tol, f"{what} g_w0")
    touched = np.unique(dev.X[ids].indices)
    cold = np.setdiff1d(np.arange(n), np.union1d(touched, hot_cols))
    assert not G_V[cold].any() and not g_w[cold].any(), f"{what}: an untouched column is not exactly zero"
    return touched


def check_records(rec, g, dev, touched, hot_cols, fixed, what):
    """A record list against the dense gradient of the same rows."""
    from conftest import rel_err
    n, k = dev.n, dev.k
    want_cols = np.union1d(touched, hot_cols)  # (a shard that is not empty lists every hot column)
    assert rec.count == len(want_cols) <= rec.cap, (what, rec.count, len(want_cols))
    r = rec.filled()
    cols = r[:, 0].astype(np.int64)
    np.testing.assert_array_equal(r[:, 0], cols.astype(np.float64))
    assert np.all(np.diff(cols) > 0), f"{what}: records do not ascend strictly"
    np.testing.assert_array_equal(cols, want_cols)
    G_V, g_w, g_w0 = split_grad(g, n, k)
    if fixed:  # every sum of a step has a fixed order: two calls give the same bits
        np.testing.assert_array_equal(r[:, 1: k + 1], G_V[cols], err_msg=f"{what} G_V")
        np.testing.assert_array_equal(r[:, k + 1], g_w[cols], err_msg=f"{what} g_w")
        assert rec.gw0 == g_w0, what
    else:
        assert rel_err(r[:, 1: k + 1], G_V[cols]) < 1e-13, what
        assert rel_err(r[:, k + 1], g_w[cols]) < 1e-13, what
        assert abs(rec.gw0 - g_w0) <= 1e-13 * max(abs(g_w0), 1e-300), what
    rec.assert_rest_untouched()


def check_all_forms(dev, params, full_ids, shard_ids, oracle_full, oracle_shard, fixed):
    """On ONE plan, in this order: dense gradient of the full batch, of the shard, then the records
    of the full batch, of the shard."""
    hot_cols = dev.plan.hot_columns()
    g_full, _ = dense_grad(dev, full_ids, params)
    g_shard, _ = dense_grad(dev, shard_ids, params)
    rec_full = grad_rows(dev, full_ids, params, dev.n)
    rec_shard = grad_rows(dev, shard_ids, params, dev.n)
    t_full = check_dense(g_full, dev, full_ids, oracle_full, hot_cols, "full batch")
    t_shard = check_dense(g_shard, dev, shard_ids, oracle_shard, hot_cols, "shard")
    check_records(rec_full, g_full, dev, t_full, hot_cols, fixed, "full batch records")
    check_records(rec_shard, g_shard, dev, t_shard, hot_cols, fixed, "shard records")


def grad_oracle(log, ids, w0, w, V):
    return fm_gradients_ld(log["features"][ids], log["labels"][ids], log["pscores"][ids], w0, w, V)
