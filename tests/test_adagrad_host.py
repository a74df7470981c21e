"""The AdaGrad rule of the FM fit, without a GPU: a float64 restatement of the fit on
cpu_ref.fm_gradients against the golden the reference produced with an AdaGrad subclass of its
BaseOptimizer (tests/golden/make_golden_adagrad.py), the intervals of adagrad_common.py -- a float64
pass in another summation order stays inside, four wrong rules are caught on the affected elements
alone --, the condition that keeps those intervals from hiding a failure on every case list of
test_gpu_adagrad.py, and the kinds of the header against the Python pair."""
import numpy as np
import pytest

import adagrad_common as ac
import grad_forms_common as gf
from conftest import assert_elementwise, rel_err
from oracle import cpu_ref
from relevance_factorizationmachine_amd import _lib

NAMES = ("w0", "w", "V", "acc_w0", "acc_w", "acc_V", "train_loss", "val_loss")


# --------------------------------------------------------------------------
# the golden
# --------------------------------------------------------------------------
@pytest.mark.parametrize("est", ["IPS", "Naive"])
def test_float64_fit_matches_the_reference_with_an_adagrad_subclass(golden, est):
    g = golden("fm_adagrad_coat_k8")
    train, val = ac.coat_split(est)
    assert str(g[f"{est}_input_digest"]) == ac.log_digest(train, val), "synthetic inputs drifted"
    got = ac.fit_f64(train, val, int(g["n_epochs"]), 8, float(g["lr"]), float(g["eps"]), float(g["init"]), 500,
                     int(g["seed"]))
    assert g[f"{est}_train_loss"][0] > 2 * g[f"{est}_train_loss"][-1]  # the fit learned
    for name in NAMES:
        want = g[f"{est}_{name}"]
        assert rel_err(got[name], want) < 1e-9, (name, rel_err(got[name], want))
        assert_elementwise(got[name], want, what=f"{est} {name}")


# --------------------------------------------------------------------------
# one step in float64 against the intervals
# --------------------------------------------------------------------------
def _one_step_f64(log, ids, theta, G, lr, eps, rule=ac.rule_f64):
    X, y, p = log["features"], log["labels"], log["pscores"]
    _, g_w0, g_w, G_V = cpu_ref.fm_gradients(X[ids], y[ids], p[ids], *theta)
    new = [rule(t, a, g, lr, eps) for t, a, g in zip(theta, G, (np.array([g_w0]), g_w, G_V))]
    return [n[0] for n in new], [n[1] for n in new]


@pytest.mark.parametrize("kind", ac.ACC_KINDS)
@pytest.mark.parametrize("batch", ["full", "shard"])
@pytest.mark.parametrize("k", [3, 16])
def test_float64_step_in_shuffled_order_stays_inside(k, batch, kind):
    log, theta, ids, oracle = ac.case_a(k)
    G = ac.acc_init(kind, *theta[2].shape, k)
    shuffled = np.random.default_rng(k).permutation(ids[batch])
    new_t, new_G = _one_step_f64(log, shuffled, theta, G, ac.LR, ac.EPS)
    ac.assert_inside(new_t, new_G, theta, G, oracle[batch], ac.LR, ac.EPS, len(shuffled), f"k={k} {batch} {kind}")
    cold = ac.assert_untouched_bitwise(new_t, new_G, theta, G, log["features"], ids[batch])
    assert len(cold) >= 3


def _touched(oracle):
    """Elements whose gradient has a term (w0 [1], w [n], V [n, k])."""
    return [np.atleast_1d(np.asarray(S) > 0) for S in oracle[3]]


def _mutation_masks(rule, eps=ac.EPS, k=16):
    log, theta, ids, oracle = ac.case_a(k)
    G = ac.acc_init("uniform", *theta[2].shape, k)
    new_t, new_G = _one_step_f64(log, ids["full"], theta, G, ac.LR, eps, rule)
    return ac.outside(new_t, new_G, theta, G, oracle["full"], ac.LR, eps, len(ids["full"])), _touched(oracle["full"])


def test_mutation_denominator_from_the_old_accumulator_is_caught():
    def rule(theta, G, g, lr, eps):
        return theta - (lr * g) / (np.sqrt(G) + eps), G + g * g
    masks, touched = _mutation_masks(rule)
    for (bad_t, bad_G), t in zip(masks, touched):
        assert np.array_equal(bad_t.reshape(t.shape), t) and not bad_G.any()


def test_mutation_eps_inside_the_root_is_caught():
    """At eps = 1e-10 and G of order one the two placements differ by 5e-11 of the step, less than
    what the tolerance of g moves it by; the mutation is run at eps = 1e-3, where they differ by
    5e-4 of the step on every element (|g| = (1 - eps) / 2 to nine digits aside)."""
    def rule(theta, G, g, lr, eps):
        Gn = G + g * g
        return theta - (lr * g) / np.sqrt(Gn + eps), Gn
    masks, touched = _mutation_masks(rule, eps=1e-3)
    for (bad_t, bad_G), t in zip(masks, touched):
        assert np.array_equal(bad_t.reshape(t.shape), t) and not bad_G.any()


def test_mutation_one_accumulator_per_row_is_caught():
    def rule(theta, G, g, lr, eps):
        if g.ndim < 2:
            return ac.rule_f64(theta, G, g, lr, eps)
        rows = (g != 0).any(axis=1)
        Gn = np.where(rows[:, None], G[:, :1] + (g * g).sum(axis=1, keepdims=True), G)
        return theta - (lr * g) / (np.sqrt(Gn) + eps), Gn
    masks, touched = _mutation_masks(rule)
    for i, ((bad_t, bad_G), t) in enumerate(zip(masks, touched)):
        if i < 2:
            assert not bad_t.any() and not bad_G.any()
        else:
            assert np.array_equal(bad_t, t) and np.array_equal(bad_G, t)


@pytest.mark.parametrize("what", ["parameter", "accumulator"])
def test_mutation_untouched_column_moves_is_caught(what):
    """One unit in the last place: inside the widened interval, so the bitwise check has to see it."""
    log, theta, ids, oracle = ac.case_a(16)
    G = ac.acc_init("uniform", *theta[2].shape, 16)
    new_t, new_G = _one_step_f64(log, ids["shard"], theta, G, ac.LR, ac.EPS)
    cold = ac.assert_untouched_bitwise(new_t, new_G, theta, G, log["features"], ids["shard"])
    hit = new_t if what == "parameter" else new_G
    hit[2][cold[-1], 3] = np.nextafter(hit[2][cold[-1], 3], np.inf)
    with pytest.raises(AssertionError, match="untouched " + what):
        ac.assert_untouched_bitwise(new_t, new_G, theta, G, log["features"], ids["shard"])
    ac.assert_inside(new_t, new_G, theta, G, oracle["shard"], ac.LR, ac.EPS, 5)


# --------------------------------------------------------------------------
# the intervals cannot hide a failure: every case list of test_gpu_adagrad.py
# --------------------------------------------------------------------------
def _condition(theta, G, oracle, rows, exempt_allowed=True):
    """The worst half-width / |step| of a case; exempt elements (adagrad_common's docstring): none
    where not allowed, else at most 1 % of an array's touched ones (fewer than half on a shard)."""
    g_w0, g_w, G_V, Ss = oracle
    worst = 0.0
    for t, a, g, S in zip(theta, G, (g_w0, g_w, G_V), Ss):
        w, n_exempt, n_touched = ac.interval_condition(t, a, g, S, ac.LR, ac.EPS, rows)
        assert exempt_allowed or n_exempt == 0, (n_exempt, n_touched)
        assert n_exempt * 2 < n_touched if rows == 5 else n_exempt * 100 <= n_touched, (n_exempt, n_touched)
        worst = max(worst, w)
    return worst


@pytest.mark.parametrize("k", sorted({k for k, _ in ac.CASES_A}), ids=gf.class_id)
def test_interval_condition_on_the_shape_classes(k):
    log, theta, ids, oracle = ac.case_a(k)
    for batch in ("full", "shard"):
        for kind in ac.ACC_KINDS:
            worst = _condition(theta, ac.acc_init(kind, *theta[2].shape, k), oracle[batch], len(ids[batch]),
                               exempt_allowed=not (k in (3, 16, 400) and kind == "zero"))
            print(f"k={k} {batch} {kind}: half-width / |step| = {worst:.3g}")
            assert worst <= 1e-5, (batch, kind, worst)


@pytest.mark.parametrize("k,hot,form", ac.CASES_SPLIT, ids=[f"{gf.class_id(k)}-{f}" for k, _, f in ac.CASES_SPLIT])
def test_interval_condition_on_the_split_columns(k, hot, form):
    log, theta, full, oracle = ac.case_split(k, form)
    for kind in ac.ACC_KINDS:
        worst = _condition(theta, ac.acc_init(kind, *theta[2].shape, k), oracle, len(full))
        print(f"k={k} {form} {kind}: half-width / |step| = {worst:.3g}")
        assert worst <= 1e-5, (kind, worst)


def test_interval_condition_on_the_hot_overflow():
    log, theta, full, oracle, _, _ = ac.case_overflow()
    for kind in ac.ACC_KINDS:
        assert _condition(theta, ac.acc_init(kind, *theta[2].shape, ac.K_OVERFLOW), oracle, len(full)) <= 1e-5


@pytest.mark.parametrize("k", ac.KS_THREE_STEPS)
def test_interval_condition_on_three_steps(k):
    """The GPU test starts each step's oracle from the device's previous state; here from the float64
    state, which the device's lies within its intervals of."""
    log = ac.log_a(False)
    theta = gf.perturbed_init(k, log["features"].shape[1], k)
    G = ac.acc_init("zero", *theta[2].shape, k)
    for ids in ac.three_batches(k):
        assert _condition(theta, G, gf.grad_oracle(log, ids, *theta), len(ids)) <= 1e-5
        theta, G = _one_step_f64(log, ids, theta, G, ac.LR, ac.EPS)


# --------------------------------------------------------------------------
# the host rule of the handle, and the kinds of the ABI
# --------------------------------------------------------------------------
def test_host_update_rule_of_the_handle():
    from relevance_factorizationmachine_amd.optimizer import adagrad_update
    rng = np.random.default_rng(3)
    p, G, g = rng.standard_normal((6, 4)), rng.uniform(0, 2, (6, 4)), rng.standard_normal((6, 4))
    want_p, want_G = ac.rule_f64(p, G, g, 0.05, 1e-10)
    q, H = p.copy(), G.copy()
    adagrad_update(q, H, g, 0.05, 1e-10)
    assert np.array_equal(q, want_p) and np.array_equal(H, want_G)
    q, H = p.copy(), G.copy()
    idx = (np.array([1, 4]), 2)  # the reference's _update_V: (columns, factor)
    adagrad_update(q, H, g[idx], 0.05, 1e-10, idx)
    keep = np.ones(p.shape, bool)
    keep[idx] = False
    assert np.array_equal(q[idx], want_p[idx]) and np.array_equal(H[idx], want_G[idx])
    assert np.array_equal(q[keep], p[keep]) and np.array_equal(H[keep], G[keep])


def test_optimizer_kinds_are_the_headers():
    """``RFM_FM_OPT_*`` of include/rfm_hip.h are the Python pair (the declarations: test_host_abi.py)."""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "rfm_hip.h")).read()
    assert int(re.search(r"#define RFM_FM_OPT_SGD (\d+)", header).group(1)) == _lib.OPT_SGD == ac.SGD
    assert int(re.search(r"#define RFM_FM_OPT_ADAGRAD (\d+)", header).group(1)) == _lib.OPT_ADAGRAD == ac.ADAGRAD
