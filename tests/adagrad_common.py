"""Shared by the tests of the FM fit's AdaGrad rule (test_adagrad_host.py, test_gpu_adagrad.py): the
rule in NumPy float64 and in long double (optimizer_common.py), the intervals a device value has to lie in, the case lists
of the GPU tests with their oracle (no GPU needed to build them, so the host test can check the
condition below on every one), a float64 restatement of the fit, and thin wrappers of the raw ABI.
Importing this module touches neither the GPU nor the package under test.

The rule, per element with accumulator G and batch-SUM gradient g:
    G_new = G + g * g,    theta_new = theta - step(g),    step(g) = lr * g / (sqrt(G + g^2) + eps).

Tolerance (derived, not measured).  step is non-decreasing in g: its derivative is
(G + eps * sqrt(G + g^2)) / (sqrt(G + g^2) * (sqrt(G + g^2) + eps)^2) >= 0.  The device's g lies within
tau = grad_forms_common.grad_tol(rows) * S of the long-double oracle's g (S: the sum of the
magnitudes of the terms of g, `fm_gradients_ld`), so
    theta_new in [theta - step(g + tau), theta - step(g - tau)],
widened by 2^-50 * (|theta| + max |step|) for the five roundings of the float64 evaluation (g * g,
the sum, the root, the sum with eps -- each moves step by at most 2^-53 relative -- then lr * g, the
quotient and the final difference), and
    G_new in [G + max(|g| - tau, 0)^2, G + (|g| + tau)^2], widened by 2^-51 relative (two roundings).
So that an interval cannot hide a wrong rule, its half-width must be at most 1e-5 * |step(g)| on
every touched element (`interval_condition`); test_adagrad_host.py asserts that for every case list
below.

Two kinds of element cannot meet that condition under any test, and are EXEMPT from it (still held
to their intervals, and counted by `interval_condition`):
- the step is at the rounding level of theta: where the residuals of the rows that hold a column
  are nearly zero (a saturated score), |step(g)| comes down to a few units in the last place of
  theta (k = 1, the 5-row shard: g = -4.9e-13 at theta = -3.8).  Criterion: the rounding allowance
  2^-50 * (|theta| + |step|) alone exceeds half of 1e-5 * |step(g)|.
- the gradient cancels: |g| < 2e-6 * S, so that tau, what the tolerance of the gradient forms leaves
  open about g, is more than half of 1e-5 * |g| (k = 511, 36 000 elements of V: a handful).  It
  matters with G > 0 only; with G = 0 the step is lr * sign(g) whatever |g|.  Criterion: tau > 0.5e-5
  * |g| and the half-width condition fails.
The host test allows at most 1 % of an array's touched elements exempt on a full batch, fewer than
half on the 5-row shards (one saturated row there is a fifth of the batch: 8 of the 21 touched
elements of w at k = 1), and none at k = 3, 16 and 400 with zero accumulators."""
import functools

import numpy as np
from scipy.sparse import csr_matrix

import grad_forms_common as gf
from optimizer_common import ADAGRAD, LD, SGD, log_digest, rule_f64, rule_ld  # noqa: F401 (the tests' names for them)
from oracle import cpu_ref

LR = 2.0 ** -3
EPS = 1e-10
EMPTY_ROWS = (5, 700, 1499)
SHARD = np.array([11, 5, 1200, 42, 977], dtype=np.int32)  # row 5 is empty
K_SHORT_SPLIT = 8


# --------------------------------------------------------------------------
# the rule
# --------------------------------------------------------------------------
def step_ld(g, G, lr, eps):
    """step(g) in long double: what the shared rule takes off theta."""
    return -rule_ld(0.0, G, g, lr, eps)[0]


def intervals(theta, G, g, S, lr, eps, rows):
    """(theta_lo, theta_hi, G_lo, G_hi, step) in long double for one parameter array; g, S: the
    oracle's gradient and magnitude sum, broadcast to theta's shape."""
    theta, G = np.asarray(theta).astype(LD), np.asarray(G).astype(LD)
    g, S = np.broadcast_to(np.asarray(g).astype(LD), theta.shape), np.broadcast_to(np.asarray(S).astype(LD), theta.shape)
    tau = LD(gf.grad_tol(rows)) * S
    st, s_hi, s_lo = step_ld(g, G, lr, eps), step_ld(g + tau, G, lr, eps), step_ld(g - tau, G, lr, eps)
    widen = LD(2.0) ** -50 * (np.abs(theta) + np.maximum(np.abs(s_hi), np.abs(s_lo)))
    G_lo = (G + np.maximum(np.abs(g) - tau, 0) ** 2)
    G_hi = (G + (np.abs(g) + tau) ** 2)
    rel = LD(2.0) ** -51
    return (theta - s_hi - widen, theta - s_lo + widen, G_lo - rel * np.abs(G_lo), G_hi + rel * np.abs(G_hi), st)


def interval_condition(theta, G, g, S, lr, eps, rows):
    """(largest half-width of a theta interval relative to |step(g)| over the touched elements (S > 0)
    that are not exempt, exempt elements, touched elements); see the module's docstring."""
    lo, hi, _, _, st = intervals(theta, G, g, S, lr, eps, rows)
    touched = np.broadcast_to(np.asarray(S) > 0, lo.shape)
    mag = np.abs(st)
    allowance = LD(2.0) ** -50 * (np.abs(np.asarray(theta).astype(LD)) + mag)
    gL = np.broadcast_to(np.asarray(g).astype(LD), lo.shape)
    tau = LD(gf.grad_tol(rows)) * np.broadcast_to(np.asarray(S).astype(LD), lo.shape)
    fails = (hi - lo) / 2 > LD(1e-5) * mag
    exempt = touched & ((allowance > LD(0.5e-5) * mag) | ((tau > LD(0.5e-5) * np.abs(gL)) & fails))
    held = touched & ~exempt
    if not held.any():
        return 0.0, int(exempt.sum()), int(touched.sum())
    return float(np.max(((hi - lo) / 2)[held] / mag[held])), int(exempt.sum()), int(touched.sum())


def outside(got_theta, got_G, theta, G, oracle, lr, eps, rows):
    """Per parameter array (w0, w, V): boolean masks (theta outside, G outside) of the device's
    values against the intervals.  NaN counts as outside."""
    g_w0, g_w, G_V, (S_0, S_w, S_V) = oracle
    out = []
    for x, a, t, G0, g, S in zip(got_theta, got_G, theta, G, (g_w0, g_w, G_V), (S_0, S_w, S_V)):
        lo, hi, G_lo, G_hi, _ = intervals(t, G0, g, S, lr, eps, rows)
        x, a = np.asarray(x, dtype=np.float64).astype(LD), np.asarray(a, dtype=np.float64).astype(LD)
        assert x.shape == lo.shape and a.shape == lo.shape, (x.shape, a.shape, lo.shape)
        out.append((~((x >= lo) & (x <= hi)), ~((a >= G_lo) & (a <= G_hi))))
    return out


def assert_inside(got_theta, got_G, theta, G, oracle, lr, eps, rows, what=""):
    for name, (bad_t, bad_G) in zip(("w0", "w", "V"), outside(got_theta, got_G, theta, G, oracle, lr, eps, rows)):
        assert not bad_t.any(), f"{what} {name}: {int(bad_t.sum())} parameters outside, first {np.argwhere(bad_t)[:3].tolist()}"
        assert not bad_G.any(), f"{what} acc_{name}: {int(bad_G.sum())} accumulators outside, first {np.argwhere(bad_G)[:3].tolist()}"


def assert_untouched_bitwise(got_theta, got_G, theta, G, X, ids, what="", some=True):
    """Columns no batch row holds keep the bits of w, V and of their accumulators (some: the case is
    meant to have such columns)."""
    n = X.shape[1]
    cold = np.setdiff1d(np.arange(n), np.unique(X[np.asarray(ids, dtype=np.int64)].indices))
    assert len(cold) > 0 or not some, "the case has no untouched column"
    for i in (1, 2):
        assert np.array_equal(np.asarray(got_theta[i])[cold], np.asarray(theta[i])[cold]), f"{what}: an untouched parameter moved"
        assert np.array_equal(np.asarray(got_G[i])[cold], np.asarray(G[i])[cold]), f"{what}: an untouched accumulator moved"
    return cold


def acc_init(kind, n, k, seed):
    """The accumulators a case starts from: 'zero', or 'uniform' in [0.25, 4]."""
    if kind == "zero":
        return np.zeros(1), np.zeros(n), np.zeros((n, k))
    rng = np.random.default_rng(1000 + seed)
    return rng.uniform(0.25, 4, size=1), rng.uniform(0.25, 4, size=n), rng.uniform(0.25, 4, size=(n, k))


# --------------------------------------------------------------------------
# the cases (the `_log_a` recipe of test_gpu_grad_forms.py, restated: that file is a GPU test)
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def log_a(small):
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
def case_a(k):
    """Log, parameters, the two batches and their oracle gradients: computed once, never modified."""
    log = log_a(k >= 500)
    n_rows, n = log["features"].shape
    theta = gf.perturbed_init(k, n, k)
    full = np.random.default_rng(k).permutation(n_rows).astype(np.int32)
    shard = SHARD % n_rows
    assert log["features"][int(shard[1])].nnz == 0
    return log, theta, {"full": full, "shard": shard}, {"full": gf.grad_oracle(log, full, *theta),
                                                        "shard": gf.grad_oracle(log, shard, *theta)}


CASES_A = [(k, hot) for k in sorted(gf.CLASS_OF) if k != 33 for hot in ((0,) if gf.chunked(k) else (0, -1, -2, 4))]
ACC_KINDS = ("zero", "uniform")
# split columns of both forms, and the hot-class overflow: (factor count, hot mode, form)
CASES_SPLIT = [(k, hot, form) for k, hot in gf.CASES_B for form in ("short", "long")]
K_OVERFLOW = 64
# three steps on one plan (both parities of the chunked bitmap); the fixed-order classes of test 3
KS_THREE_STEPS = (65, 400)
CASES_FIXED = [(k, hot) for k, hot in CASES_A if gf.fixed_order(k, hot) and k in (3, 8, 16, 32, 63, 128, 65, 400)]
THREE_BATCH = 400


@functools.lru_cache(maxsize=None)
def case_split(k, form):
    bc = gf.full_batch_workgroup_slots(k)
    n_rows = (bc if form == "short" else K_SHORT_SPLIT * bc) + 37
    assert n_rows <= gf.GRAD_TOL_ROWS
    log, theta, full, shard = gf.split_case(k, n_rows, 24 if n_rows > 5000 else 60, 1, 7 * k + len(form))
    return log, theta, full, gf.grad_oracle(log, full, *theta)


@functools.lru_cache(maxsize=None)
def case_overflow():
    k = K_OVERFLOW
    hot_cap = min(160, (56 << 10) // ((k + 2) * 8))
    n_rows, n_cols, dense = gf.full_batch_workgroup_slots(k) + 37, 150, hot_cap + 7
    log, theta, full, shard = gf.split_case(k, n_rows, n_cols, dense, 64)
    return log, theta, full, gf.grad_oracle(log, full, *theta), hot_cap, dense


def three_batches(k):
    n_rows = log_a(False)["features"].shape[0]
    rng = np.random.default_rng(k)
    return [rng.permutation(n_rows)[:THREE_BATCH].astype(np.int32) for _ in range(3)]


# --------------------------------------------------------------------------
# the fit, restated in float64 on cpu_ref.fm_gradients
# --------------------------------------------------------------------------
def fit_f64(train, val, n_epochs, n_factors, lr, eps, init, batch_size, seed, order=None, mutate=None):
    """src/fm.py:55-112 with the AdaGrad rule: dict of final parameters, accumulators, loss lists.
    order: a permutation generator (rng) -- the batch rows are summed in a shuffled order;
    mutate(theta, G, g, lr, eps) -> (theta_new, G_new): another rule (the mutation tests)."""
    X, y, p = train["features"].tocsr(), train["labels"], train["pscores"]
    w0, w, V = cpu_ref.fm_init(seed, X.shape[1], n_factors)
    G = [np.full(a.shape, float(init)) for a in (w0, w, V)]
    rule = mutate or rule_f64
    tr, va = [], []
    for epoch in range(n_epochs):
        rows = cpu_ref.batch_ids(X.shape[0], batch_size, epoch)
        if order is not None:
            rows = rows[order.permutation(len(rows))]
        Xb, yb, pb = X[rows], y[rows], p[rows]
        _, g_w0, g_w, G_V = cpu_ref.fm_gradients(Xb, yb, pb, w0, w, V)
        new = [rule(t, a, g, lr, eps) for t, a, g in zip((w0, w, V), G, (np.array([g_w0]), g_w, G_V))]
        (w0, w, V), G = [n[0] for n in new], [n[1] for n in new]
        rows = cpu_ref.batch_ids(X.shape[0], batch_size, epoch)
        tr.append(cpu_ref.ips_logloss(y[rows], cpu_ref.fm_predict(X[rows], w0, w, V), p[rows]))
        va.append(cpu_ref.ips_logloss(val["labels"], cpu_ref.fm_predict(val["features"], w0, w, V), val["pscores"]))
    return {"w0": w0, "w": w, "V": V, "acc_w0": G[0], "acc_w": G[1], "acc_V": G[2], "train_loss": np.array(tr),
            "val_loss": np.array(va)}


def coat_split(est):
    from relevance_factorizationmachine_amd import synth
    return synth.make_log(synth.SHAPES["coat"], "FM", est, seed=0)


# --------------------------------------------------------------------------
# the raw ABI
# --------------------------------------------------------------------------
def set_optimizer(dev, kind, accs=None, eps=EPS):
    """rfm_fm_plan_set_optimizer on a gf.DeviceLog's plan; accs: a gf.Params of (acc_w0, acc_w, acc_V)."""
    from relevance_factorizationmachine_amd import _lib
    ptrs = accs.ptrs() if accs is not None else (None, None, None)
    return dev.rt.lib.rfm_fm_plan_set_optimizer(dev.plan.handle, kind, *ptrs, eps)


def optimizer_of(dev):
    from relevance_factorizationmachine_amd import _lib
    out = np.full(1, -7, dtype=np.int32)
    _lib.check(dev.rt.lib.rfm_fm_plan_optimizer(dev.plan.handle, out.ctypes.data))
    return int(out[0])


def adagrad_step(dev, ids, params, accs, lr=LR, eps=EPS):
    """One rfm_fm_step under AdaGrad; asserts the plan reports the rule."""
    from relevance_factorizationmachine_amd import _lib
    _lib.check(set_optimizer(dev, ADAGRAD, accs, eps))
    assert optimizer_of(dev) == ADAGRAD
    gf.step(dev, ids, params, lr)
    return params.host(), accs.host()
