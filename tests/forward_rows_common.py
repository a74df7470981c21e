"""Shared by the row-by-row tests of the FM forward (test_forward_oracle_host.py,
test_gpu_forward_rows.py): the long-double row oracle with the magnitude every logit adds up, the
three tolerances derived from it, the logs whose rows sit at the edges of a workgroup's trip, and
thin wrappers of the raw ABI calls (rfm_fm_forward, rfm_fm_forward_loss, rfm_fm_train and the two
host-only queries rfm_fm_forward_geometry / rfm_fm_train_forms).  Importing this module touches
neither the GPU nor the package under test.

The oracle (``row_oracle``) works on the entries of the CSR, row groups of equal length at a time,
so that a row of 5 * 64 + 3 entries does not make every row of its log pay for 300 dense columns;
test_forward_oracle_host.py holds it to grad_forms_common.fm_logit_ld on the dense matrix.  For
each row it gives the logit z, the clipped logit, the score p and

    S_z = |w0| + sum_c |w_c x_c| + 1/2 sum_f (sum_c |v_cf x_c|)^2 + 1/2 sum_{c,f} (v_cf x_c)^2,

the sum of the absolute values of everything the row's logit adds up.  With u = 2^-53:

logit   |dz| <= (2 L + K + 16) u S_z, L the row's length, K the factor count.  A factor sum of L
        rounded products is off by at most L u of its absolute sum; squaring doubles that; the
        K-term sum over the factors, in any order, adds K u; 16 covers the lane-group tree, the
        linear term and the final adds.
score   |dp| <= p (1 - p) tol_z (1 + tol_z) + 8 u p: the logit's error through the sigmoid's slope,
        and 3 ulp of exp (the OpenCL bound the device library is built to) with the add and the
        divide.  Rows whose oracle score is not finite must be non-finite, all others finite.
loss    (mean IPS log-loss of n rows, r = y / pscore): per row
        tau = |r| tol_p / (p + eps) + |1 - r| tol_p / (1 - p + eps)
              + 4 u (|r log(p + eps)| + |(1 - r) log(1 - p + eps)|),
        and the mean gets (sum tau + n u sum |term|) / n.

All three are derived, not measured: on the CPU the float64 reference, in its own and in a shuffled
order, stays below half of each (test_forward_oracle_host.py).

Inputs: parameters in the style of grad_forms_common.perturbed_init (w0 = 0.37, every w_c off zero)
with V scaled so that at least 80 % of a log's rows score inside (1e-6, 1 - 1e-6) -- a saturated
sigmoid would hide the logit; the host test asserts it for every log.  A log has 48 columns where
its longest row (5 lanes-per-row + 3 entries) fits them, else 5 lanes-per-row + 8."""
import functools

import numpy as np
from scipy.sparse import csr_matrix

import grad_forms_common as gf
from oracle import cpu_ref

LD = np.longdouble
U = 2.0 ** -53
EPS = cpu_ref.LOSS_EPS
CLIP = cpu_ref.LOGIT_CLIP


# --------------------------------------------------------------------------
# the oracle
# --------------------------------------------------------------------------
class Rows:
    """What ``row_oracle`` gives, one element per row (np.longdouble; ``length`` int64)."""

    def __init__(self, z, S_z, length):
        self.z, self.S_z, self.length = z, S_z, length
        self.zc = np.where(np.isnan(z), z, np.clip(z, -LD(CLIP), LD(CLIP)))
        with np.errstate(over="ignore"):
            self.p = 1 / (1 + np.exp(-self.zc))

    def take(self, rows):
        out = Rows.__new__(Rows)
        for name in ("z", "S_z", "length", "zc", "p"):
            setattr(out, name, getattr(self, name)[rows])
        return out


def row_oracle(X, w0, w, V):
    """Logit, S_z and length of every row of the CSR matrix X (its entries as they are stored: no
    sorting, no merging), in np.longdouble, rows of equal length together."""
    indptr, cols, x = X.indptr.astype(np.int64), X.indices, X.data.astype(LD)
    n_rows = len(indptr) - 1
    w0 = LD(np.asarray(w0, dtype=np.float64).reshape(-1)[0])
    w, V = np.asarray(w).astype(LD), np.asarray(V).astype(LD)
    k = V.shape[1]
    length = np.diff(indptr)
    z = np.full(n_rows, w0, dtype=LD)
    S = np.full(n_rows, abs(w0), dtype=LD)
    for L in np.unique(length):
        if L == 0:
            continue
        rows = np.flatnonzero(length == L)
        step = max(1, int(2_000_000 // (L * k)))  # rows at a time: [step, L, k] long doubles
        for at in range(0, len(rows), step):
            rr = rows[at: at + step]
            e = indptr[rr][:, None] + np.arange(L)[None, :]
            xc, cc = x[e], cols[e]
            vx = V[cc] * xc[:, :, None]                   # [m, L, k]
            q = vx.sum(axis=1)
            sq = (vx * vx).sum(axis=(1, 2))
            z[rr] = w0 + (w[cc] * xc).sum(axis=1) + ((q * q).sum(axis=1) - sq) / 2
            aq = np.abs(vx).sum(axis=1)
            S[rr] = abs(w0) + np.abs(w[cc] * xc).sum(axis=1) + ((aq * aq).sum(axis=1) + sq) / 2
    return Rows(z, S, length)


# --------------------------------------------------------------------------
# the tolerances
# --------------------------------------------------------------------------
def tol_z(o, k):
    return (2 * o.length + k + 16).astype(LD) * LD(U) * o.S_z


def tol_p(o, k):
    tz = tol_z(o, k)
    return o.p * (1 - o.p) * tz * (1 + tz) + 8 * LD(U) * o.p


def loss_oracle(o, k, y, pscore, eps=EPS):
    """Mean IPS log-loss of the rows of ``o`` in long double, and its tolerance."""
    r = np.asarray(y).astype(LD) / np.asarray(pscore).astype(LD)
    a, b = r * np.log(o.p + LD(eps)), (1 - r) * np.log(1 - o.p + LD(eps))
    tp = tol_p(o, k)
    tau = (np.abs(r) * tp / (o.p + LD(eps)) + np.abs(1 - r) * tp / (1 - o.p + LD(eps))
           + 4 * LD(U) * (np.abs(a) + np.abs(b)))
    n = len(r)
    term = a + b
    return -term.sum() / n, (tau.sum() + n * LD(U) * np.abs(term).sum()) / n


def score_excess(got, o, k):
    """|got - p| / tol_p per row (inf where finiteness disagrees; 0 where both are non-finite)."""
    got = np.asarray(got, dtype=np.float64)
    want_finite = np.isfinite(o.p)
    with np.errstate(invalid="ignore"):
        ratio = np.abs(got.astype(LD) - o.p) / tol_p(o, k)
    ratio = np.where(want_finite & np.isfinite(got), ratio, np.inf)
    return np.where(~want_finite & ~np.isfinite(got), 0.0, ratio).astype(np.float64)


def assert_scores(got, o, k, what, bound=1.0):
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == o.p.shape, (what, got.shape, o.p.shape)
    ex = score_excess(got, o, k)
    bad = ~(ex <= bound)
    if bad.any():
        i = int(np.argmax(np.where(bad, ex, -1)))
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} rows outside {bound} * tol_p; worst row {i} "
                             f"(length {int(o.length[i])}): got {got[i]!r}, want {float(o.p[i])!r}, "
                             f"|d| / tol_p {ex[i]!r}, z {float(o.z[i])!r}")


def assert_loss(got, want, tol, what, bound=1.0):
    assert np.isfinite(got) and abs(LD(got) - want) <= bound * tol, \
        f"{what}: loss {got!r}, want {float(want)!r}, |d| {float(abs(LD(got) - want))!r}, tolerance {float(tol)!r}"


# --------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------
def n_cols_for(lpr):
    return 48 if 5 * lpr + 3 <= 48 else 5 * lpr + 8


def row_lengths(lpr):
    return np.array([0, 1, lpr - 1, lpr, lpr + 1, 2 * lpr, 2 * lpr + 1])


def forward_params(seed, n, k, lpr):
    """perturbed_init with V scaled: the pair term of a row of L entries of unit variance has a
    standard deviation of sigma_v^2 L sqrt(K / 2); about 3 at L = 2 lpr + 1."""
    w0, w, V = gf.perturbed_init(seed, n, k)
    sigma2 = V.var()
    V = V * np.sqrt(3.0 / (sigma2 * (2 * lpr + 1) * np.sqrt(max(k, 2) / 2)))
    return w0, w, V


def forward_log(seed, n_rows, lpr, w0, w, empties=(), pairs=(), max_len=None, n_cols=None, rare=0, long_share=0.1,
                special=None):
    """A log of ``n_rows`` rows of 0, 1, lpr - 1, lpr, lpr + 1, 2 lpr, 2 lpr + 1 entries (the five
    longer lengths a share ``long_share`` of the rows each; ``max_len``: none longer), distinct
    ascending columns in a row.

    - rows ``empties`` (and the first and the last) are empty;
    - ``pairs`` = (a, b): row a is the long row of 5 lpr + 3 entries (at most max_len), on column 0
      and the last column among others, row b is empty;
    - ``special`` single-entry rows after the first have their x set for logits of +-750 (past the
      clip) and +-40 (the pair term of a single entry is exactly zero): eight by default, two of
      each kind, four in a log of fewer than 100 rows, where eight would be more than a fifth of
      the rows; 0: none (their x runs into the thousands and dwarfs every other term of a sum);
    - the last ``rare`` columns are drawn so rarely that each has about ten entries in the log."""
    rng = np.random.default_rng(seed)
    n_cols = n_cols_for(lpr) if n_cols is None else n_cols
    assert len(w) == n_cols
    lens = row_lengths(lpr)
    prob = np.array([0.4 * (1 - 5 * long_share), 0.6 * (1 - 5 * long_share)] + [long_share] * 5)
    if max_len is not None:
        prob = np.where(lens <= max_len, prob, 0.0)
    length = rng.choice(lens, size=n_rows, p=prob / prob.sum())
    long_len = min(5 * lpr + 3, max_len if max_len is not None else 1 << 30)
    special = np.arange(1, 1 + ((8 if n_rows >= 100 else 4) if special is None else special))
    assert n_rows >= 12 and not set(special) & (set(empties) | {a for a, _ in pairs} | {b for _, b in pairs})
    length[special] = 1
    for a, b in pairs:
        length[a], length[b] = long_len, 0
    length[list(empties) + [0, n_rows - 1]] = 0
    indptr = np.concatenate([[0], np.cumsum(length)]).astype(np.int64)
    cols = np.empty(indptr[-1], dtype=np.int32)
    weight = np.ones(n_cols)
    if rare:
        assert long_len <= n_cols - rare
        weight[n_cols - rare:] = min(1.0, 10.0 * (n_cols - rare) / max(int(indptr[-1]), 1))
    for L in np.unique(length):
        if L == 0:
            continue
        rows = np.flatnonzero(length == L)
        # (weighted draws without replacement: the L smallest of -log(u) / weight)
        keys = -np.log(rng.random((len(rows), n_cols))) / weight[None, :]
        pick = np.sort(np.argsort(keys, axis=1)[:, :L], axis=1)
        cols[(indptr[rows][:, None] + np.arange(L)[None, :])] = pick
    for a, _ in pairs:  # (the long rows: column 0 and the last column in use)
        if long_len >= 2:
            cols[indptr[a]], cols[indptr[a + 1] - 1] = 0, n_cols - 1
    x = rng.standard_normal(indptr[-1])
    targets = np.array([750.0, -750.0, 40.0, -40.0, 750.0, -750.0, 40.5, -39.5])
    at = indptr[special]
    x[at] = (targets[: len(special)] - w0[0]) / w[cols[at]]
    X = csr_matrix((x, cols, indptr), shape=(n_rows, n_cols))
    y = (rng.random(n_rows) < 0.5).astype(np.int64)
    p = rng.uniform(0.1, 1.0, size=n_rows) ** 0.5
    return {"features": X, "labels": y, "pscores": p}


def unsaturated_share(o):
    p = o.p[np.isfinite(o.p)]
    return float(np.mean((p > 1e-6) & (p < 1 - 1e-6)))


# --------------------------------------------------------------------------
# the cases of test_gpu_forward_rows.py whose inputs do not depend on the device: the host test
# checks the condition and the float64 reference on exactly these
# --------------------------------------------------------------------------
HOST_ROWS = 1200   # rows of a log of the host test (the device tests: more of the same kind)
LOSS_CLASSES = (8, 32, 128, 300, 513)  # lpr 4, 16, 64, nc 3, nc 16


@functools.lru_cache(maxsize=None)
def case(k, n_rows, empties=(), pairs=(), max_len=None, seed=0, lpr=None, rare=0, special=None):
    """Log, parameters and row oracle of a factor count: computed once, shared, never modified.
    The parameters depend on the factor count and the column count alone (logs of different
    ``seed`` share them: a training log and its validation log).  ``lpr``: the lanes per row of a
    factor count that CLASS_OF does not list.  A log bounded by ``max_len`` has max_len + 8
    columns, and ``rare`` rare ones behind them.  ``special``: see forward_log."""
    lpr = gf.CLASS_OF[k][0] if lpr is None else lpr
    n = n_cols_for(lpr) if max_len is None else max(48, max_len + 8) + rare
    theta = forward_params(1000 + k, n, k, lpr)
    # (the widest factor counts: fewer long rows, so that the oracle of a pass of rows stays at
    # seconds)
    log = forward_log(7 * k + seed, n_rows, lpr, theta[0], theta[1], empties, pairs, max_len, n, rare,
                      0.1 if k < 500 else 0.04, special)
    return log, theta, row_oracle(log["features"], *theta)


# --------------------------------------------------------------------------
# the raw ABI calls
# --------------------------------------------------------------------------
def forward_geometry(rt, n_rows, k, records):
    """rfm_fm_forward_geometry -> dict(block, grid, trip, lpr)."""
    from relevance_factorizationmachine_amd import _lib
    out = np.zeros(4, dtype=np.int32)
    _lib.check(rt.lib.rfm_fm_forward_geometry(rt.ctx, int(n_rows), int(k), int(bool(records)), out.ctypes.data))
    return dict(zip(("block", "grid", "trip", "lpr"), (int(v) for v in out)))


def many_rows_minimum(rt, k, records):
    """The smallest row count whose forward takes the 1 024-thread shape (by bisection on the query:
    the shape is monotone in the row count)."""
    lo, hi = 1, 1 << 22
    assert forward_geometry(rt, hi, k, records)["block"] == 1024
    while lo < hi:
        mid = (lo + hi) // 2
        if forward_geometry(rt, mid, k, records)["block"] == 1024:
            hi = mid
        else:
            lo = mid + 1
    return lo


FORM_NAMES = ("sliced", "merged", "scores_only", "ride", "ride_val", "run_len", "train_block", "val_block")


def train_forms(rt, plan, batch, n_iters, call_iters, val, n_val, want_train=True, want_val=True):
    """rfm_fm_train_forms -> dict of FORM_NAMES; ``val`` a DeviceRows or None."""
    from relevance_factorizationmachine_amd import _lib
    out = np.zeros(8, dtype=np.int32)
    ptrs = val.csr_ptrs() if val is not None else (None,) * 3
    _lib.check(rt.lib.rfm_fm_train_forms(rt.ctx, plan.handle, batch, n_iters, call_iters, *ptrs, n_val,
                                         int(want_train), int(want_val), out.ctypes.data))
    return dict(zip(FORM_NAMES, (int(v) for v in out)))


class DeviceRows:
    """A CSR with labels and propensities on the device, for the forwards through the caller's arrays."""

    def __init__(self, rt, log):
        from relevance_factorizationmachine_amd.runtime import DeviceCSR
        self.rt = rt
        self.csr = DeviceCSR(rt, log["features"])
        self.y = rt.upload(log["labels"], dtype=np.float64)
        self.p = rt.upload(log["pscores"], dtype=np.float64)
        self.n_rows, self.n = log["features"].shape

    def csr_ptrs(self):
        c = self.csr
        return c.indptr.data_ptr(), c.indices.data_ptr(), c.values.data_ptr()


def forward(rt, dev, params, n_rows, ids=None):
    """rfm_fm_forward of rows ids[0 .. n_rows) (or 0 .. n_rows) into a NaN-filled buffer with guard
    elements behind it."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    d_ids = rt.upload(np.asarray(ids, dtype=np.int32)) if ids is not None else None
    out = torch.full((n_rows + gf.GUARD,), float("nan"), dtype=torch.float64, device=rt.torch_device)
    _lib.check(rt.lib.rfm_fm_forward(rt.ctx, *dev.csr_ptrs(), d_ids.data_ptr() if ids is not None else None, n_rows,
                                     *params.ptrs(), dev.n, params.k, out.data_ptr()))
    rt.sync()
    got = out.cpu().numpy()
    assert np.isnan(got[n_rows:]).all(), "a score past the rows of the launch was written"
    return got[:n_rows]


def forward_loss(rt, dev, params, n_rows, ids=None, with_pred=True, eps=EPS):
    """rfm_fm_forward_loss -> (loss, scores or None)."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    d_ids = rt.upload(np.asarray(ids, dtype=np.int32)) if ids is not None else None
    out = torch.full((n_rows + gf.GUARD,), float("nan"), dtype=torch.float64, device=rt.torch_device)
    loss = torch.full((1 + gf.GUARD,), float("nan"), dtype=torch.float64, device=rt.torch_device)
    _lib.check(rt.lib.rfm_fm_forward_loss(
        rt.ctx, *dev.csr_ptrs(), dev.y.data_ptr(), dev.p.data_ptr(), d_ids.data_ptr() if ids is not None else None,
        n_rows, *params.ptrs(), dev.n, params.k, eps, out.data_ptr() if with_pred else None, loss.data_ptr()))
    rt.sync()
    got, lo = out.cpu().numpy(), loss.cpu().numpy()
    assert np.isnan(got[n_rows:]).all() and np.isnan(lo[1:]).all()
    if not with_pred:
        assert np.isnan(got).all()
    return float(lo[0]), (got[:n_rows] if with_pred else None)


def train_lr0(rt, dev, params, ids, val, part_call_iters=None, want_train=True, want_val=True, eps=EPS):
    """rfm_fm_train (or rfm_fm_train_part) with lr = 0 on ``dev`` (a grad_forms_common.DeviceLog) for
    the batches ids [n_iters, batch], validation log ``val`` (a DeviceRows) -> per-iteration
    (train losses, validation losses); asserts that w0, w, V keep their bits."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    n_iters, batch = ids.shape
    d_ids = rt.upload(ids.reshape(-1))
    before = params.host()
    tl = torch.full((n_iters + gf.GUARD,), float("nan"), dtype=torch.float64, device=rt.torch_device)
    vl = torch.full((n_iters + gf.GUARD,), float("nan"), dtype=torch.float64, device=rt.torch_device)
    args = [rt.ctx, dev.plan.handle, *dev.log_ptrs(), d_ids.data_ptr(), batch, n_iters, *params.ptrs(), 0.0,
            *val.csr_ptrs(), val.y.data_ptr(), val.p.data_ptr(), val.n_rows, eps,
            tl.data_ptr() if want_train else None, vl.data_ptr() if want_val else None]
    if part_call_iters is None:
        _lib.check(rt.lib.rfm_fm_train(*args))
    else:
        _lib.check(rt.lib.rfm_fm_train_part(*args, part_call_iters))
    rt.sync()
    for a, b, name in zip(params.host(), before, ("w0", "w", "V")):
        np.testing.assert_array_equal(a, b, err_msg=f"a call with lr = 0 changed {name}")
    t, v = tl.cpu().numpy(), vl.cpu().numpy()
    assert np.isnan(t[n_iters:]).all() and np.isnan(v[n_iters:]).all()
    return t[:n_iters], v[:n_iters]
