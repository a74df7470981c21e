"""Shared by the tests of FM fold-in (test_fm_fold_host.py, test_gpu_fm_fold.py): a long-double
statement of the fold-in semantics (the reference's batch-sum step, src/fm.py:80-88
with :135-187, restricted to the new row's id column), one row at a time; an f64 restatement with the
examples and the dot products summed in the opposite order; case builders with a chosen geometry, the
case list, a small coat-shaped catalogue for the Python flows, and thin wrappers of the raw ABI calls
that keep every float array on the device between sentinels.  Importing this module touches neither
the GPU nor the library under test.

The rule.  New row r has fixed feature sums g_r, l_r, a trained id column (omega_r, nu_r) and examples
e that name rows j_e of the fixed side F, fL with weights ry_e; c is w0.  One pass:
    h_e = g_r + F[j_e];  z_e = c + l_r + fL[j_e] + g_r.F[j_e] + omega_r + nu_r.h_e
    err_e = ry_e - sigmoid(clip(z_e));  omega_r += lr sum_e err_e;  nu_r += lr sum_e err_e h_e
with every err_e taken before the update.

Comparison.  Folded factor rows are compared element by element against the largest magnitude of THEIR
OWN ROW in the oracle, weights against max(|want|, lr) (``mf_step_common.row_distance`` /
``bias_distance``); the served operands A = g + nu and L = l + omega + g.nu on the same scales.

Step size.  A full-batch step is not contractive by itself: the Jacobian of one pass is
I - lr sum_e s'(z_e) (1, h_e)(1, h_e)^T with s' <= 1/4, so every case takes the largest power of two
``lr`` with lr * n_max * (1 + max_e |h_e|^2) / 4 <= 1/2 (``FmFoldCase.lr``, at most ``LR_CAP``); then
a pass does not amplify a rounding error and the floor stays flat over passes.

Tolerance.  ``FMFOLD_TOL`` is not taken from a device result.  ``FMFOLD_FLOOR`` is the distance of the
f64 restatement from the long-double oracle on those scales, over every case of the list
(test_fm_fold_host.py measures it on the CPU and holds the constant within 5%).
``FMFOLD_TOL = min(64 * FMFOLD_FLOOR, 1e-11)``; the factor 64 is the project's margin for the device's
exp, division and FMA contraction (``MF_TOL``, ``FOLD_TOL``).  The smallest error a wrong read makes (a
skipped example, a stale nu) is lr * |err| * |h| of a row that is itself a sum of such terms: orders
above the tolerance (the mutation tests).  Measured floor: 2.7e-15 (factor rows 2.6e-15, the row of
1 029 examples at k = 8; weights 1.2e-15), so ``FMFOLD_TOL`` = 1.7e-13.  Largest distance an MI355X
showed over the case list and the flows: 1.4e-15 (``GPU_MAX_SEEN``), below the CPU floor and 120 times
inside ``FMFOLD_TOL``."""
import functools
import types
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp

import fold_common
import mf_step_common as ms
from fold_common import FOLD_BLOCK, GRID_PER_CU, LD, N_FIXED, _chains, _sigmoid
from mf_step_common import Guarded, PAD

FMFOLD_FLOOR = 2.7e-15                # measured CPU floor to two digits (test_tolerance_floor holds it within 5%)
FMFOLD_TOL = min(64 * FMFOLD_FLOOR, 1e-11)
GPU_MAX_SEEN = 1.4e-15                # largest distance an MI355X showed over the case list (shape-k3)

LONG_ROW = 1029                       # the long row of the narrowest classes
C0 = 0.4                              # w0 of every case
LR_CAP = 0.05


def pad4(k):
    return (int(k) + 3) // 4 * 4


def groups(k):
    """Lane groups of a workgroup = examples of a row in flight."""
    return FOLD_BLOCK // ms.shape_class(k)[0]


# --------------------------------------------------------------------------
# the semantics: one row, pass by pass (the form the mutations are made in)
# --------------------------------------------------------------------------
def _sum_rows_reversed(a):
    """Sum over the first axis, strictly from the last example to the first."""
    return np.cumsum(a[::-1], axis=0)[-1]


def fold_row(ids, ry, F, fL, g, l, c, nu0, om0, n_passes, lr, dtype=LD, reverse=False, mutation=None):
    """The id column of one new row after ``n_passes`` passes: ``(nu [k], omega)`` in ``dtype``.
    ``F`` is ``[n_fixed, >= k]`` (columns past k are ignored).  ``reverse``: examples, factors and the
    logit's terms summed in the opposite order.  ``mutation`` breaks the rule in one of four ways
    (test_fm_fold_host.py): "skips_last" = the last example is left out; "err_after_omega" = the
    error that moves nu is taken after omega has moved; "no_g_in_h" = h_e = F[j_e]; "stale_nu" = from
    the second pass on the logit reads the nu from before the previous pass."""
    ids = np.asarray(ids, dtype=np.int64)
    k = len(np.asarray(g))
    n = len(ids) - (mutation == "skips_last" and len(ids) > 0)
    ids = ids[:n]
    ry = np.asarray(ry).astype(dtype)[:n]
    Fj = np.asarray(F)[ids][:, :k].astype(dtype)
    fl = np.asarray(fL)[ids].astype(dtype)
    g = np.asarray(g).astype(dtype)
    nu, om = np.array(nu0, dtype=dtype), dtype(om0)
    l, c, lr = dtype(l), dtype(c), dtype(lr)
    h = Fj if mutation == "no_g_in_h" else g + Fj
    dot = ms._dot_reversed if reverse else (lambda a, b: (a * b).sum(axis=-1))
    total = _sum_rows_reversed if reverse else (lambda a: a.sum(axis=0))
    before = nu
    for p in range(n_passes if n else 0):
        seen = before if (mutation == "stale_nu" and p >= 1) else nu
        before = nu
        if reverse:
            z = dot(seen, h) + om + dot(g, Fj) + fl + l + c
        else:
            z = c + l + fl + dot(g, Fj) + om + dot(seen, h)
        err = ry - _sigmoid(z, dtype)
        om_new = om + lr * total(err)
        if mutation == "err_after_omega":
            err = ry - _sigmoid(z - om + om_new, dtype)
        nu = nu + lr * total(err[:, None] * h)
        om = om_new
    return nu, om


def served(g, l, nu, om):
    """The operands the grown row is served with: ``(A [kpad], L)`` in the dtype of ``nu``."""
    dtype = np.asarray(nu).dtype.type
    g = np.asarray(g).astype(dtype)
    A = np.zeros(pad4(len(g)), dtype=dtype)
    A[: len(g)] = g + nu
    return A, dtype(l) + dtype(om) + (g * nu).sum()


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------
@dataclass
class FmFoldCase(fold_common.FoldCaseBase):
    def fixed(self):
        """The fixed side ``(F [n_fixed, k], fL [n_fixed])``: rows of squared length about 1."""
        rng = self._rng("fixed-")
        F = rng.uniform(-1.0, 1.0, size=(self.n_fixed, self.k)) * np.sqrt(3.0 / self.k)
        fL = rng.normal(scale=0.3, size=self.n_fixed)
        if self.clip:
            fL[0], fL[1] = 900.0, -900.0
        return F, fL

    def feature_sums(self):
        """The new rows' own ``(g [n_new, k], l [n_new])``: rows of squared length about 1/4."""
        rng = self._rng("sums-")
        return (rng.uniform(-1.0, 1.0, size=(self.n_new, self.k)) * np.sqrt(0.75 / self.k),
                rng.normal(scale=0.2, size=self.n_new))

    def start(self):
        """Initial ``(nu [n_new, k], omega [n_new])``: zeros, or a caller's values."""
        if not self.with_init:
            return np.zeros((self.n_new, self.k)), np.zeros(self.n_new)
        rng = self._rng("init-")
        return (rng.uniform(-1.0, 1.0, size=(self.n_new, self.k)) * np.sqrt(0.75 / self.k),
                rng.normal(scale=0.1, size=self.n_new))

    def step_bound(self):
        """n_max * (1 + max_e |h_e|^2) / 4: what ``lr`` times must stay within 1/2."""
        if not self.lengths.sum():
            return 0.0
        F, _ = self.fixed()
        g, _ = self.feature_sums()
        h = np.repeat(g, self.lengths, axis=0) + F[self.ids]
        return float(self.lengths.max() * (1.0 + (h * h).sum(axis=1).max()) / 4.0)

    @functools.cached_property
    def lr(self):
        return _lr_for(self.step_bound())


def _lr_for(bound):
    """The largest power of two with lr * bound <= 1/2, at most LR_CAP."""
    if bound <= 0.0:
        return LR_CAP
    return float(min(LR_CAP, 2.0 ** np.floor(np.log2(0.5 / bound))))


def fold_all(case, dtype=LD, reverse=False, start=None, n_passes=None):
    """Every new row of a case after its passes, row by row: ``(nu [n_new, k], omega [n_new])``."""
    F, fL = case.fixed()
    g, l = case.feature_sums()
    nu0, om0 = case.start() if start is None else start
    ry, ptr = case.ry(), case.row_ptr
    n_passes = case.n_passes if n_passes is None else n_passes
    V, w = np.zeros((case.n_new, case.k), dtype=dtype), np.zeros(case.n_new, dtype=dtype)
    for r in range(case.n_new):
        sl = slice(ptr[r], ptr[r + 1])
        V[r], w[r] = fold_row(case.ids[sl], ry[sl], F, fL, g[r], l[r], C0, nu0[r], om0[r], n_passes, case.lr,
                              dtype=dtype, reverse=reverse)
    return V, w


def served_all(case, V, w):
    """``(A [n_new, kpad], L [n_new])`` of folded columns, in their dtype."""
    g, l = case.feature_sums()
    dtype = np.asarray(V).dtype
    A, L = np.zeros((case.n_new, pad4(case.k)), dtype=dtype), np.zeros(case.n_new, dtype=dtype)
    for r in range(case.n_new):
        A[r], L[r] = served(g[r], l[r], V[r], w[r])
    return A, L


SHAPE_KS = ms.SHAPE_KS                       # the lowest and highest k of the 19 classes, 300 and 400
NARROW_KS = (1, 2, 3, 8)                     # the classes of four lanes per example: 64 lane groups
PASS_KS = (2, 33, 400, 1024)
COUNT_KS = (8, 130)
SPECIAL_KS = (7, 130)
ASSUMED_GRID = ms.ASSUMED_CUS * GRID_PER_CU  # workgroups of the null-context geometry


def edge_lengths(k):
    """Example counts around the lane groups of a workgroup."""
    gpb = groups(k)
    return [gpb + 1, 0, 2 * gpb + 1, 1, gpb - 1, gpb]


def shape_case(k):
    """a. rows of 0, 1, GPB-1, GPB, GPB+1 and 2 GPB+1 examples side by side, two passes; at four
    lanes per example one row of 1 029."""
    lengths = edge_lengths(k) + ([LONG_ROW, 2] if k in NARROW_KS else [])
    name = f"shape-k{k}"
    return FmFoldCase(name, k, _chains(name, lengths), 2)


def pass_case(k, n_passes):
    """b. the same rows under 0, 1, 2, 3 passes (0: from a caller's init, which must keep its bits)."""
    return FmFoldCase(f"passes{n_passes}-k{k}", k, _chains(f"passes-k{k}", edge_lengths(k) + [3, 2]), n_passes,
                      with_init=(n_passes == 0))


def count_cases(k):
    """c. 1, one short of the grid, the grid and one more rows than the null-context grid has
    workgroups, 0..2 examples each.  The rows start from a caller's values of order 1: among
    thousands of rows started at zero a few end where two examples' terms cancel, and a comparison
    relative to the row's own magnitude then measures that cancellation, not the arithmetic."""
    out = []
    for n in (1, ASSUMED_GRID - 1, ASSUMED_GRID, ASSUMED_GRID + 1):
        name = f"count{n}-k{k}"
        rng = np.random.default_rng(n + k)
        flat = rng.integers(0, N_FIXED, size=3 * n)
        chains = [flat[3 * r: 3 * r + (r * 7 + 2) % 3] for r in range(n)]
        out.append(FmFoldCase(name, k, chains, 2, with_init=True))
    return out


def special_case(k, with_init):
    """d. a row that names a fixed row twice in succession and again later; a fixed row (5) in
    every row; logits driven past the clip on both sides (fixed rows 0, 1); a caller's init."""
    chains = [np.array([5, 7, 7, 3, 7, 9]), np.array([5, 0, 0, 4]), np.array([1, 5, 1]), np.array([5]),
              np.array([6, 5, 6, 6, 5, 5, 2, 6, 0, 1, 5])]
    return FmFoldCase(f"special{'-init' if with_init else ''}-k{k}", k, chains, 3, with_init=with_init, clip=True)


@functools.lru_cache(maxsize=None)
def fold_cases():
    out = [shape_case(k) for k in SHAPE_KS]
    out += [pass_case(k, p) for k in PASS_KS for p in (0, 1, 2, 3)]
    for k in COUNT_KS:
        out += count_cases(k)
    out += [special_case(k, init) for k in SPECIAL_KS for init in (False, True)]
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return {c.name: c for c in out}


oracle = fold_common.cached_oracle(fold_cases, fold_all)  # (nu, omega) in long double


def distance(got, want, lr):
    """(largest factor-row distance, largest weight distance) of ``got = (V, w)`` from the oracle."""
    rows = ms.row_distance(got[0], want[0]) if np.asarray(got[0]).size else np.zeros(1)
    bias = ms.bias_distance(got[1], want[1], lr) if np.asarray(got[1]).size else np.zeros(1)
    return float(rows.max()), float(bias.max())


def floor_of(case):
    return distance(fold_all(case, dtype=np.float64, reverse=True), oracle(case), case.lr)


def assert_within(got, want, tol, what, lr):
    """``(rows [n, m], scalars [n])`` against the oracle's, element by element.  Returns the largest distance."""
    worst = 0.0
    if np.asarray(got[0]).size:
        worst = max(ms.assert_rows_within(got[0], want[0], tol, f"{what} rows"),
                    ms.assert_bias_within(got[1], want[1], tol, f"{what} scalars", lr))
    return worst


# --------------------------------------------------------------------------
# the side sums on the host, and a small coat-shaped catalogue for the flows
# --------------------------------------------------------------------------
def side_sums_np(X, w, V, dtype=np.float64):
    """``(A [n, k], L [n])`` of a side matrix: rfm_fm_side_sums restated (recommend.py's identity)."""
    D = np.asarray(X.todense()).astype(dtype)
    w, V = np.asarray(w).astype(dtype), np.asarray(V).astype(dtype)
    A = D @ V
    return A, D @ w + 0.5 * ((A * A).sum(axis=1) - ((D * D) @ (V * V)).sum(axis=1))


FLOW_USERS, FLOW_ITEMS, FLOW_UW, FLOW_IW, FLOW_NEW = 12, 9, 4, 3, 5
FLOW_LENGTHS = (6, 0, 3, 11, 2)
FLOW_FIT = dict(n_epochs=3, lr=0.05, batch_size=40, alpha=0.3)


@functools.lru_cache(maxsize=None)
def flow_problem(k, side="user", seed=5):
    """A catalogue in the layout of ``fm_features_coat`` -- [one-hot user | user table | one-hot item |
    item table] -- with 12 users and 9 items, a training log on it, and ``FLOW_NEW`` rows that arrive
    after the fit on ``side``: their table rows (no id column) and their first interactions."""
    rng = np.random.default_rng(1000 * seed + k + (side == "item"))
    nu, ni, uw, iw = FLOW_USERS, FLOW_ITEMS, FLOW_UW, FLOW_IW

    def table(n, width):
        T = (rng.random((n, width)) < 0.6).astype(np.float64)
        T[:, 0] = 1.0  # (no row without a feature)
        return T

    UT, IT = table(nu, uw), table(ni, iw)
    n_features = nu + uw + ni + iw
    XU = sp.hstack([sp.identity(nu), sp.csr_matrix(UT), sp.csr_matrix((nu, ni + iw))]).tocsr()
    XI = sp.hstack([sp.csr_matrix((ni, nu + uw)), sp.identity(ni), sp.csr_matrix(IT)]).tocsr()
    n = 80
    users, items = rng.integers(0, nu, size=n), rng.integers(0, ni, size=n)
    train = {"features": (XU[users] + XI[items]).tocsr(), "labels": (rng.random(n) < 0.5).astype(np.int64),
             "pscores": rng.uniform(0.1, 1.0, size=n) ** 0.5}
    val = {key: v[:20] for key, v in train.items()}
    NT = table(FLOW_NEW, uw if side == "user" else iw)
    if side == "user":
        new_rows = sp.hstack([sp.csr_matrix((FLOW_NEW, nu)), sp.csr_matrix(NT), sp.csr_matrix((FLOW_NEW, ni + iw))]).tocsr()
    else:
        new_rows = sp.hstack([sp.csr_matrix((FLOW_NEW, nu + uw + ni)), sp.csr_matrix(NT)]).tocsr()
    n_fixed = ni if side == "user" else nu
    m = int(sum(FLOW_LENGTHS))
    new = np.repeat(np.arange(FLOW_NEW), FLOW_LENGTHS)
    other = rng.integers(0, n_fixed, size=m)
    take = rng.permutation(m)  # the rows' examples arrive interleaved
    cols = (new, other) if side == "user" else (other, new)
    data = {"features": np.stack(cols, axis=1)[take], "labels": (rng.random(m) < 0.5).astype(np.float64)[take],
            "pscores": (rng.uniform(0.1, 1.0, size=m) ** 0.5)[take]}
    return types.SimpleNamespace(k=k, side=side, seed=seed, n_features=n_features, XU=XU, XI=XI, train=train, val=val,
                                 new_rows=new_rows, data=data, n_new=FLOW_NEW, n_fixed=n_fixed, n_passes=3)


def flow_fit(prob):
    """The small fit of the flows: the CPU oracle's, ``(w0, w, V)``."""
    from oracle import cpu_ref
    ref = cpu_ref.fm_fit(prob.train, prob.val, n_factors=prob.k, seed=prob.seed, with_losses=False, **FLOW_FIT)
    return ref["w0"], ref["w"], ref["V"]


def flow_operands(prob, w, V, dtype=np.float64):
    """``(g, l, F, fL)`` of a flow: the new rows' feature sums and the fixed other side."""
    g, l = side_sums_np(prob.new_rows, w, V, dtype)
    F, fL = side_sums_np(prob.XI if prob.side == "user" else prob.XU, w, V, dtype)
    return g, l, F, fL


def flow_grouped(prob):
    """The flow's examples as the kernel takes them: ``(row_ptr, ids, ry)``, a row's examples in input order."""
    col = 0 if prob.side == "user" else 1
    pairs = prob.data["features"]
    by_row = np.argsort(pairs[:, col], kind="stable")
    counts = np.bincount(pairs[:, col], minlength=prob.n_new)
    ry = (prob.data["labels"] / prob.data["pscores"])[by_row]
    return np.concatenate([[0], np.cumsum(counts)]), pairs[by_row, 1 - col], ry


def flow_lr(prob, w, V):
    g, _, F, _ = flow_operands(prob, w, V)
    ptr, ids, _ = flow_grouped(prob)
    h = np.repeat(g, np.diff(ptr), axis=0) + F[ids]
    return _lr_for(float(np.diff(ptr).max() * (1.0 + (h * h).sum(axis=1).max()) / 4.0))


def flow_oracle(prob, w0, w, V, lr, dtype=LD, start=None):
    """The folded id columns of a flow, ``(nu [n_new, k], omega [n_new])``, from zeros or ``start``."""
    g, l, F, fL = flow_operands(prob, w, V, dtype)
    ptr, ids, ry = flow_grouped(prob)
    nu, om = np.zeros((prob.n_new, prob.k), dtype=dtype), np.zeros(prob.n_new, dtype=dtype)
    if start is not None:
        nu[:], om[:] = start
    for r in range(prob.n_new):
        sl = slice(ptr[r], ptr[r + 1])
        nu[r], om[r] = fold_row(ids[sl], ry[sl], F, fL, g[r], l[r], w0[0], nu[r], om[r], prob.n_passes, lr, dtype=dtype)
    return nu, om


def grown_params(w, V, nu, om):
    """``(w, V)`` of the model grown by folded id columns, stored last."""
    return (np.concatenate([np.asarray(w, dtype=np.float64), np.asarray(om, dtype=np.float64)]),
            np.concatenate([np.asarray(V, dtype=np.float64), np.asarray(nu, dtype=np.float64)]))


def grown_sides(prob):
    """``(XU, XI)`` of the grown width: the new rows appended to their side with their id column."""
    pad = sp.csr_matrix
    new = sp.hstack([prob.new_rows, sp.identity(prob.n_new)]).tocsr()
    XU = sp.hstack([prob.XU, pad((prob.XU.shape[0], prob.n_new))]).tocsr()
    XI = sp.hstack([prob.XI, pad((prob.XI.shape[0], prob.n_new))]).tocsr()
    return (sp.vstack([XU, new]).tocsr(), XI) if prob.side == "user" else (XU, sp.vstack([XI, new]).tocsr())


def pair_rows(XU, XI, users, items):
    """The design matrix of the pairs ``(users[n], items[n])``."""
    return (XU[np.asarray(users)] + XI[np.asarray(items)]).tocsr()


def all_pairs(n_users, n_items, first_user=0):
    u = np.repeat(np.arange(first_user, n_users), n_items)
    return u, np.tile(np.arange(n_items), n_users - first_user)


def smallest_gap(logits):
    """The smallest gap between adjacent logits of any row."""
    s = np.sort(np.asarray(logits, dtype=np.float64), axis=1)
    return float(np.diff(s, axis=1).min())


def ranking(logits, k):
    """recommend()'s order: logit descending, ties the higher item index first."""
    return np.argsort(logits, axis=1, kind="stable")[:, ::-1][:, :k]


# --------------------------------------------------------------------------
# the raw ABI calls, every float array on the device between sentinels
# --------------------------------------------------------------------------
def geometry(n_new, k, rt=None):
    """rfm_fm_fold_geometry -> dict(lpr, vec, nc, groups, grid); ``rt`` None: no context, the grid of a
    device of 256 CUs."""
    from relevance_factorizationmachine_amd import _lib
    out = np.zeros(5, dtype=np.int32)
    _lib.check(_lib.load().rfm_fm_fold_geometry(None if rt is None else rt.ctx, int(n_new), int(k), out.ctypes.data))
    return dict(zip(("lpr", "vec", "nc", "groups", "grid"), (int(v) for v in out)))


def _padded(M, k):
    out = np.zeros((M.shape[0], pad4(k)))
    out[:, :k] = M
    return out


def run_fold(rt, case, start=None, n_passes=None):
    """rfm_fm_fold_in on a case from its start (or ``start``): ``(V, w, A, L)`` afterwards.  The
    feature sums, the fixed side, the weights, w0 and every sentinel are asserted to keep their bits."""
    from relevance_factorizationmachine_amd import _lib
    k, kp, n = case.k, pad4(case.k), case.n_new
    F, fL = case.fixed()
    g, l = case.feature_sums()
    nu0, om0 = case.start() if start is None else start
    ry = case.ry()
    n_passes = case.n_passes if n_passes is None else n_passes
    c = np.array([C0])
    inputs = [(Guarded(rt, _padded(F, k), kp), _padded(F, k), "the fixed rows"), (Guarded(rt, fL, PAD), fL, "the fixed sums"),
              (Guarded(rt, _padded(g, k), kp), _padded(g, k), "the feature sums"), (Guarded(rt, l, PAD), l, "the feature l"),
              (Guarded(rt, ry, PAD), ry, "the weights"), (Guarded(rt, c, PAD), c, "w0")]
    d_F, d_fL, d_g, d_l, d_ry, d_c = (i[0] for i in inputs)
    d_V, d_w = Guarded(rt, nu0, k), Guarded(rt, om0, PAD)
    d_A, d_L = Guarded.blank(rt, n * kp, kp), Guarded.blank(rt, n)
    ints = fold_common.upload_ints(rt, case)
    _lib.check(rt.lib.rfm_fm_fold_in(
        rt.ctx, ints[0].data_ptr(), ints[1].data_ptr(), d_ry.ptr, ints[2].data_ptr(), n, d_g.ptr, d_l.ptr, d_F.ptr,
        d_fL.ptr, case.n_fixed, d_c.ptr, k, case.lr, n_passes, d_w.ptr, d_V.ptr, d_A.ptr, d_L.ptr))
    rt.sync()
    fold_common.assert_inputs_kept(case, inputs, ints)
    return d_V.host().reshape(n, k), d_w.host(), d_A.host().reshape(n, kp), d_L.host()
