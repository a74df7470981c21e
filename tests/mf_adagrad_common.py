"""Shared by the tests of the AdaGrad rule of the exact MF batch step (test_mf_adagrad_host.py,
test_gpu_mf_adagrad.py): a long-double statement of the rule looped example by example, a float64
restatement with the dot product summed backwards (and four wrong rules), the two accumulator
states, distances, tolerances, and a wrapper of rfm_mf_sgd_levels_opt that keeps all eight device
arrays between sentinels.  The cases, builders, distances of parameters and the ``Guarded`` /
``DeviceParams`` wrappers are those of mf_step_common.py.  Importing this module touches neither the
GPU nor the library under test.

The rule (include/rfm_hip.h, "MF: the optimiser seam"; one array's update: optimizer_common.py).
Every element of P, Q, b_u, b_i has an accumulator G.  For one example (u, i), err is formed once
and then, in the reference's order,
    g = -err Q_i + reg P_u;       G_P[u] += g g;  P_u -= (lr g) / (sqrt(G_P[u]) + eps)
    g = -err P_u(new) + reg Q_i;  G_Q[i], Q_i likewise
    g = -err + reg b_u[u];        G_bu[u], b_u[u] likewise
    g = -err + reg b_i[i];        G_bi[i], b_i[i] likewise

Comparison.  Parameters as in mf_step_common (rows against the largest magnitude of their own row
in the oracle, biases against max(|want|, lr)).  An accumulator row is compared element by element
against the largest value of ITS OWN ROW in the oracle, a bias accumulator on the scale of its bias,
max(|want|, lr).  Rows and biases of users and items outside the batch keep the bits of all eight
arrays.  No element is excluded.

Tolerance.  Not taken from a device result.  ``floor_of`` runs the float64 restatement with the dot
product summed backwards and measures its distance from the long-double oracle on those scales, over
every case of ``step_cases()`` and both accumulator states (test_mf_adagrad_host.py does that on the
CPU and holds the figures below within 5 %).  ``PARAM_TOL = min(64 * PARAM_FLOOR, 1e-11)`` and
``ACC_TOL = min(64 * ACC_FLOOR, 1e-11)``: the factor of 64 is the margin ``MF_TOL`` has, for the
device's exp, division, root and FMA contraction.  No case's floor may exceed 1e-12 (asserted on the
CPU): an ill-conditioned first step, lr g / (|g| + eps) at G0 = 0 with a tiny g, would be mended in
the case's inputs, not here.  Measured floors over the case list (lr, reg, b of mf_step_common,
eps = 1e-10):

    state                    rows      biases    accumulators
    G0 = 0                   1.2e-14   1.3e-14   1.1e-13   (ring-cached-k400 / shape-k3 / shape-k1)
    G0 uniform in [0.25, 4]  2.7e-15   1.2e-14   3.0e-15

(G0 = 0 is the harder state: an element's first step is lr g / (|g| + eps) and its accumulator g g,
so both carry twice the relative error of g, which the residual's cancellation sets.)
"""
import functools

import numpy as np

import mf_step_common as ms
from mf_step_common import B0, LD, LR, REG
from optimizer_common import ADAGRAD, SGD, log_digest, rule_f64, rule_ld  # noqa: F401 (the tests' names for them)

EPS = 1e-10
ACC_KINDS = ("zero", "uniform")
ACC_SEED = 23
NAMES = ("P", "Q", "b_u", "b_i", "G_P", "G_Q", "G_bu", "G_bi")

PARAM_FLOOR = 1.3e-14   # measured CPU floor of rows and biases to two digits (the host test holds it within 5 %)
ACC_FLOOR = 1.1e-13     # ... of the accumulators
PARAM_TOL = min(64 * PARAM_FLOOR, 1e-11)
ACC_TOL = min(64 * ACC_FLOOR, 1e-11)
CASE_FLOOR_LIMIT = 1e-12
GPU_MAX_SEEN = (1.2e-14, 1.1e-13)  # largest distances an MI355X showed over the case list: a parameter
#                                    (ring-cached-k400, G0 = 0) and an accumulator (shape-k1, G0 = 0): the CPU floors


def acc_init(case, kind):
    """The four accumulators a case starts from: zeros, or uniform in [0.25, 4] from a fixed seed."""
    shapes = [np.shape(a) for a in case.init()]
    if kind == "zero":
        return tuple(np.zeros(s) for s in shapes)
    assert kind == "uniform"
    rng = np.random.default_rng(ACC_SEED)
    return tuple(rng.uniform(0.25, 4.0, size=s) for s in shapes)


# --------------------------------------------------------------------------
# the oracle: long double, example by example
# --------------------------------------------------------------------------
def mf_adagrad_batch_ld(pairs, ry, params, accs, b, lr, reg, eps, form=None):
    """One batch under the rule in np.longdouble; returns the eight arrays (P, Q, b_u, b_i and their
    accumulators).  ``form`` as in ``ms.mf_sgd_batch_ld``: "loop" walks the batch example by example,
    "disjoint" (every user and item once) updates all rows at once, None picks."""
    pairs = np.asarray(pairs, dtype=np.int64)
    P, Q, bu, bi = (np.array(a, dtype=LD) for a in params)
    GP, GQ, Gbu, Gbi = (np.array(a, dtype=LD) for a in accs)
    ry = np.asarray(ry).astype(LD)
    b, lr, reg, eps = LD(b), LD(lr), LD(reg), LD(eps)
    if form is None:
        form = "disjoint" if ms.is_disjoint(pairs) else "loop"
    if form == "disjoint":
        assert ms.is_disjoint(pairs)
        u, i = pairs[:, 0], pairs[:, 1]
        err = ry - ms._sigmoid_ld((P[u] * Q[i]).sum(axis=1) + bu[u] + bi[i] + b)
        P[u], GP[u] = rule_ld(P[u], GP[u], -err[:, None] * Q[i] + reg * P[u], lr, eps)
        Q[i], GQ[i] = rule_ld(Q[i], GQ[i], -err[:, None] * P[u] + reg * Q[i], lr, eps)
        bu[u], Gbu[u] = rule_ld(bu[u], Gbu[u], -err + reg * bu[u], lr, eps)
        bi[i], Gbi[i] = rule_ld(bi[i], Gbi[i], -err + reg * bi[i], lr, eps)
        return P, Q, bu, bi, GP, GQ, Gbu, Gbi
    assert form == "loop"
    for (u, i), r in zip(pairs, ry):
        err = r - ms._sigmoid_ld((P[u] * Q[i]).sum() + bu[u] + bi[i] + b)
        P[u], GP[u] = rule_ld(P[u], GP[u], -err * Q[i] + reg * P[u], lr, eps)
        # the item row sees the user row this example has just updated
        Q[i], GQ[i] = rule_ld(Q[i], GQ[i], -err * P[u] + reg * Q[i], lr, eps)
        bu[u], Gbu[u] = rule_ld(bu[u], Gbu[u], -err + reg * bu[u], lr, eps)
        bi[i], Gbi[i] = rule_ld(bi[i], Gbi[i], -err + reg * bi[i], lr, eps)
    return P, Q, bu, bi, GP, GQ, Gbu, Gbi


# --------------------------------------------------------------------------
# the float64 restatement (dot product summed backwards) and four wrong rules
# --------------------------------------------------------------------------
MUTATIONS = ("old_G", "eps_in_root", "stale_user_row", "row_acc")


def _rule_f64(theta, G, g, lr, eps, mutation=None):
    """One array's update in float64, the shared rule or a wrong one: returns (theta_new, G_new)."""
    if mutation == "row_acc" and np.ndim(g) >= 1 and np.ndim(G) == np.ndim(g):
        # one accumulator per row instead of per element: kept in the row's first element, read by all
        Gn = np.array(G, dtype=np.float64)
        Gn[..., :] = G[..., :1] + (g * g).sum(axis=-1, keepdims=True)
        return theta - (lr * g) / (np.sqrt(Gn) + eps), Gn
    new, Gn = rule_f64(theta, G, g, lr, eps)
    if mutation == "old_G":
        return theta - (lr * g) / (np.sqrt(G) + eps), Gn
    if mutation == "eps_in_root":
        return theta - (lr * g) / np.sqrt(Gn + eps), Gn
    return new, Gn


def mf_adagrad_batch_f64(pairs, ry, params, accs, b, lr, reg, eps, mutation=None, dot=ms._dot_reversed):
    """The same batch in float64, example by example; ``dot(p, q)`` sums the products (backwards by
    default, ``np.dot`` for the reference's own order); ``mutation``: one of ``MUTATIONS``."""
    assert mutation is None or mutation in MUTATIONS
    pairs = np.asarray(pairs, dtype=np.int64)
    P, Q, bu, bi = (np.array(a, dtype=np.float64) for a in params)
    GP, GQ, Gbu, Gbi = (np.array(a, dtype=np.float64) for a in accs)
    ry = np.asarray(ry, dtype=np.float64)
    row_mut = mutation if mutation != "stale_user_row" else None
    for (u, i), r in zip(pairs, ry):
        err = r - ms._sigmoid_f64(b + bi[i] + bu[u] + dot(P[u], Q[i]))
        p_old = P[u].copy()
        P[u], GP[u] = _rule_f64(P[u], GP[u], -err * Q[i] + reg * P[u], lr, eps, row_mut)
        p_seen = p_old if mutation == "stale_user_row" else P[u]
        Q[i], GQ[i] = _rule_f64(Q[i], GQ[i], -err * p_seen + reg * Q[i], lr, eps, row_mut)
        scal = row_mut if row_mut != "row_acc" else None
        bu[u], Gbu[u] = _rule_f64(bu[u], Gbu[u], -err + reg * bu[u], lr, eps, scal)
        bi[i], Gbi[i] = _rule_f64(bi[i], Gbi[i], -err + reg * bi[i], lr, eps, scal)
    return P, Q, bu, bi, GP, GQ, Gbu, Gbi


# --------------------------------------------------------------------------
# comparison
# --------------------------------------------------------------------------
def distances(got8, want8, lr=LR):
    """The eight distance arrays of a result against the oracle, in the order of ``NAMES``."""
    return (ms.row_distance(got8[0], want8[0]), ms.row_distance(got8[1], want8[1]),
            ms.bias_distance(got8[2], want8[2], lr), ms.bias_distance(got8[3], want8[3], lr),
            ms.row_distance(got8[4], want8[4]), ms.row_distance(got8[5], want8[5]),
            ms.bias_distance(got8[6], want8[6], lr), ms.bias_distance(got8[7], want8[7], lr))


def outside(got8, want8, lr=LR):
    """Per array, the mask of elements outside its tolerance."""
    return tuple(~(d <= LD(PARAM_TOL if j < 4 else ACC_TOL)) for j, d in enumerate(distances(got8, want8, lr)))


def assert_all_within(got8, want8, start8, pairs, what, lr=LR):
    """All eight arrays of a device against the oracle, element by element, and rows and biases of
    users and items outside the batch against the bits they started from.  Returns the largest
    distance of a parameter and of an accumulator."""
    pairs = np.asarray(pairs)
    worst = [0.0, 0.0]
    for j, (name, d) in enumerate(zip(NAMES, distances(got8, want8, lr))):
        tol = PARAM_TOL if j < 4 else ACC_TOL
        worst[j // 4] = max(worst[j // 4], ms._assert_small(d, tol, f"{what} {name}", got8[j], want8[j]))
        g, start = np.asarray(got8[j]), np.asarray(start8[j])
        rest = np.setdiff1d(np.arange(len(start)), pairs[:, j % 2])
        assert np.array_equal(g[rest].view(np.uint64), start[rest].view(np.uint64)), \
            f"{what}: a row of {name} outside the batch changed"
    return tuple(worst)


# --------------------------------------------------------------------------
# oracles and floors of the cases
# --------------------------------------------------------------------------
def oracle_of(case, kind, lr=LR, eps=EPS):
    y, p = case.ry()
    return mf_adagrad_batch_ld(case.pairs, y / p, case.init(), acc_init(case, kind), B0, lr, REG, eps)


@functools.lru_cache(maxsize=None)
def _oracle_by_name(name, kind):
    return oracle_of(ms.step_cases()[name], kind)


def oracle(case, kind):
    """The eight arrays after the batch, in long double; computed once per case and state."""
    return _oracle_by_name(case.name, kind) if case.name in ms.step_cases() else oracle_of(case, kind)


def floor_of(case, kind):
    """Distances of the float64 restatement (dot product summed backwards) from the oracle: (rows,
    biases, accumulators)."""
    y, p = case.ry()
    got = mf_adagrad_batch_f64(case.pairs, y / p, case.init(), acc_init(case, kind), B0, LR, REG, EPS)
    d = distances(got, oracle(case, kind))
    return (float(max(d[0].max(), d[1].max())), float(max(d[2].max(), d[3].max())),
            float(max(x.max() for x in d[4:])))


# --------------------------------------------------------------------------
# the raw ABI call, all eight device arrays between sentinels
# --------------------------------------------------------------------------
GEOMETRY = ("lanes_per_row", "factors_per_chunk", "chunks_per_lane", "seq_threads", "acc_ahead",
            "lds_bytes_per_cached_item", "row_ahead")


def geometry(kind, k):
    """``rfm_mf_opt_geometry`` as a dict (host only)."""
    from relevance_factorizationmachine_amd import _lib
    out = np.zeros(len(GEOMETRY), dtype=np.int32)
    _lib.check(_lib.load().rfm_mf_opt_geometry(None, int(kind), int(k), out.ctypes.data))
    return dict(zip(GEOMETRY, (int(v) for v in out)))


def assert_class(case, kind=ADAGRAD):
    """The class a case means, from the library's own geometry query."""
    geo = geometry(kind, case.k)
    lpr, vec, nc = ms.shape_class(case.k)
    assert (geo["lanes_per_row"], geo["factors_per_chunk"], geo["chunks_per_lane"]) == (lpr, vec, nc), geo
    assert geo["acc_ahead"] == 0
    assert geo["lds_bytes_per_cached_item"] == 8 * (case.k + 2) * (2 if kind == ADAGRAD else 1)
    want_threads = ms.SEQ_BLOCK_CHUNKED if nc > 1 else ms.SEQ_BLOCK
    if kind == ADAGRAD and nc > 8:
        want_threads = 256   # (the level limit stays ms.seq_cap: two passes)
    assert geo["seq_threads"] == want_threads, geo
    assert (geo["row_ahead"] > 0) == (nc <= 4) and geo["row_ahead"] <= ms.READ_AHEAD, geo
    return geo


class DeviceState:
    """The four parameters and the four accumulators on the device, every array between sentinels."""

    def __init__(self, rt, params, accs):
        self.params = ms.DeviceParams(rt, *params)
        self.accs = ms.DeviceParams(rt, *accs)

    def host(self):
        return self.params.host() + self.accs.host()


def upload_schedule(rt, sched):
    ex, lptr, cache = sched
    d_ex = rt.upload(np.ascontiguousarray(ex).view(np.uint8))
    d_lptr = rt.upload(lptr)
    d_cache = rt.upload(cache) if len(cache) else None
    return d_ex, d_lptr, d_cache


def call_opt(rt, k, sched, dev_sched, state, kind, lr=LR, eps=EPS, acc_ptrs=None, n_levels=None):
    """rfm_mf_sgd_levels_opt on a schedule of ``ms.reach`` and a ``DeviceState``; returns the code."""
    _, lptr, cache = sched
    d_ex, d_lptr, d_cache = dev_sched
    acc_ptrs = state.accs.ptrs() if acc_ptrs is None else acc_ptrs
    return rt.lib.rfm_mf_sgd_levels_opt(
        rt.ctx, d_ex.data_ptr(), lptr.ctypes.data, d_lptr.data_ptr(), len(lptr) - 1 if n_levels is None else n_levels,
        d_cache.data_ptr() if len(cache) else None, len(cache), *state.params.ptrs(), B0, k, lr, REG, int(kind),
        *acc_ptrs, eps)


def run_levels_opt(rt, case, sched, params, accs, kind=ADAGRAD, lr=LR, eps=EPS):
    """The eight arrays after rfm_mf_sgd_levels_opt on the schedule of ``ms.reach``."""
    from relevance_factorizationmachine_amd import _lib
    state = DeviceState(rt, params, accs)
    _lib.check(call_opt(rt, case.k, sched, upload_schedule(rt, sched), state, kind, lr, eps))
    return state.host()
