"""The AdaGrad rule of the exact MF batch step, without a GPU: the long-double oracle of
mf_adagrad_common.py against a float64 loop on ``optimizer.adagrad_update`` (the host rule of
``DeviceAdaGrad``), that loop against the golden the reference produced with an AdaGrad subclass of
its BaseOptimizer (tests/golden/make_golden_mf_adagrad.py), the tolerance floors and the condition
that keeps them from hiding a failure, four wrong rules caught on the affected elements and only
there, the kinds of the header against the Python pair, and the argument checks that need no
device."""
import numpy as np
import pytest

import mf_adagrad_common as ma
import mf_step_common as ms
from conftest import assert_elementwise, rel_err
from oracle import cpu_ref
from relevance_factorizationmachine_amd import _lib, synth
from relevance_factorizationmachine_amd.optimizer import adagrad_update

GOLDEN = {"IPS": "mf_adagrad_small", "Naive": "mf_adagrad_small_naive"}


# --------------------------------------------------------------------------
# the host rule of the handle, example by example
# --------------------------------------------------------------------------
def handle_loop(pairs, ry, params, accs, b, lr, reg, eps):
    """src/mf.py:97-108 with :172-216 on ``adagrad_update(params, acc, grad, lr, eps, index)``: what
    the reference runs when ``src.mf.SGD`` is an AdaGrad subclass of its BaseOptimizer."""
    P, Q, bu, bi = (np.array(a, dtype=np.float64) for a in params)
    GP, GQ, Gbu, Gbi = (np.array(a, dtype=np.float64) for a in accs)
    for (u, i), r in zip(np.asarray(pairs, dtype=np.int64), np.asarray(ry, dtype=np.float64)):
        err = r - cpu_ref.sigmoid(np.dot(P[u], Q[i]) + bu[u] + bi[i] + b)
        adagrad_update(P, GP, -err * Q[i] + reg * P[u], lr, eps, u)
        adagrad_update(Q, GQ, -err * P[u] + reg * Q[i], lr, eps, i)
        adagrad_update(bu, Gbu, -err + reg * bu[u], lr, eps, u)
        adagrad_update(bi, Gbi, -err + reg * bi[i], lr, eps, i)
    return P, Q, bu, bi, GP, GQ, Gbu, Gbi


@pytest.mark.parametrize("kind", ma.ACC_KINDS)
@pytest.mark.parametrize("name", ["shape-k3", "shape-k16", "ring-cached-k16", "ring-uncached-k128", "limit-cache-k400"])
def test_oracle_against_the_handles_own_rule(name, kind):
    case = ms.step_cases()[name]
    y, p = case.ry()
    start = case.init() + ma.acc_init(case, kind)
    got = handle_loop(case.pairs, y / p, start[:4], start[4:], ms.B0, ms.LR, ms.REG, ma.EPS)
    worst = ma.assert_all_within(got, ma.oracle(case, kind), start, case.pairs, f"{name} {kind}")
    print(f"{name} {kind}: parameters {worst[0]:.3g}, accumulators {worst[1]:.3g}")


@pytest.mark.parametrize("est", ["IPS", "Naive"])
def test_float64_fit_matches_the_reference_with_an_adagrad_subclass(golden, est):
    g = golden(GOLDEN[est])
    sh = synth.SHAPES["kuairec_small"]
    train, val = synth.make_log(sh, "MF", est, seed=0)
    assert str(g[f"{est}_input_digest"]) == ma.log_digest(train, val), "synthetic inputs drifted"
    k, B, lr, reg, eps = int(g["n_factors"]), int(g["batch_size"]), float(g["lr"]), float(g["reg"]), float(g["eps"])
    X, y, p = train["features"], train["labels"], train["pscores"]
    state = cpu_ref.mf_init(int(g["seed"]), sh.n_users, sh.n_items, k)
    state = tuple(state) + tuple(np.full(np.shape(a), float(g["init"])) for a in state)
    b = float(np.mean(y))
    assert b == float(g[f"{est}_b"])
    tr, va = [], []
    for epoch in range(int(g["n_epochs"])):
        rows = cpu_ref.batch_ids(X.shape[0], B, epoch)
        state = handle_loop(X[rows], y[rows] / p[rows], state[:4], state[4:], b, lr, reg, eps)
        tr.append(cpu_ref.ips_logloss(y[rows], cpu_ref.mf_predict(X[rows], *state[:4], b), p[rows]))
        va.append(cpu_ref.ips_logloss(val["labels"], cpu_ref.mf_predict(val["features"], *state[:4], b), val["pscores"]))
    assert g[f"{est}_train_loss"][0] > g[f"{est}_train_loss"][-1]  # the fit learned
    got = dict(zip(("P", "Q", "b_u", "b_i", "acc_P", "acc_Q", "acc_b_u", "acc_b_i"), state), train_loss=tr, val_loss=va)
    for name, have in got.items():
        want = g[f"{est}_{name}"]
        assert rel_err(have, want) < 1e-12, (name, rel_err(have, want))
        assert_elementwise(have, want, rtol=1e-12, atol=1e-15, what=f"{est} {name}")


# --------------------------------------------------------------------------
# the floors, and the condition that no case hides behind them
# --------------------------------------------------------------------------
def test_tolerance_floors_and_condition():
    worst = {kind: [0.0, 0.0, 0.0] for kind in ma.ACC_KINDS}
    for name, case in ms.step_cases().items():
        for kind in ma.ACC_KINDS:
            f = ma.floor_of(case, kind)
            assert max(f) <= ma.CASE_FLOOR_LIMIT, (name, kind, f)  # else: change the case's inputs
            worst[kind] = [max(a, b) for a, b in zip(worst[kind], f)]
    for kind, (rows, bias, acc) in worst.items():
        print(f"floor {kind}: rows {rows:.2e} biases {bias:.2e} accumulators {acc:.2e}")
    params = max(max(w[0], w[1]) for w in worst.values())
    accs = max(w[2] for w in worst.values())
    assert abs(params / ma.PARAM_FLOOR - 1) <= 0.05, (params, ma.PARAM_FLOOR)
    assert abs(accs / ma.ACC_FLOOR - 1) <= 0.05, (accs, ma.ACC_FLOOR)
    assert ma.PARAM_TOL == 64 * ma.PARAM_FLOOR < 1e-11 and ma.ACC_TOL == 64 * ma.ACC_FLOOR < 1e-11


def test_grid_case_floor():
    """The one case the GPU test builds from the device's CU count, at the count the host assumes."""
    for k in ms.GRID_KS:
        case = ms.grid_case(k, 8)  # (8 CUs: the floor of one wide level does not depend on its length)
        for kind in ma.ACC_KINDS:
            assert max(ma.floor_of(case, kind)) <= ma.CASE_FLOOR_LIMIT


# --------------------------------------------------------------------------
# four wrong rules, each caught on the affected elements and only there
# --------------------------------------------------------------------------
MUT_K, MUT_N = 16, 150


def _mutation_masks(mutation, eps=ma.EPS):
    """One level of MUT_N disjoint examples (no error is carried to another example) from the
    uniform accumulator state: per array the elements outside the tolerance, and the touched rows."""
    users, items = ms.concat(ms.disjoint(MUT_N), skip0=True)
    case = ms.Case("mutation", MUT_K, users, items, {})
    y, p = case.ry()
    start = case.init() + ma.acc_init(case, "uniform")
    want = ma.mf_adagrad_batch_ld(case.pairs, y / p, start[:4], start[4:], ms.B0, ms.LR, ms.REG, eps)
    right = ma.mf_adagrad_batch_f64(case.pairs, y / p, start[:4], start[4:], ms.B0, ms.LR, ms.REG, eps)
    assert not any(m.any() for m in ma.outside(right, want))
    got = ma.mf_adagrad_batch_f64(case.pairs, y / p, start[:4], start[4:], ms.B0, ms.LR, ms.REG, eps, mutation)
    touched = []
    for j, a in enumerate(start):
        t = np.zeros(np.shape(a), dtype=bool)
        t[case.pairs[:, j % 2]] = True
        touched.append(t)
    return ma.outside(got, want), touched


def _assert_caught(masks, touched, affected):
    """An affected array: nothing outside the tolerance but elements of touched rows, and at least
    95 % of those (the rest belong to examples whose residual or gradient is so small that the wrong
    rule moves them by less than the tolerance).  Any other array: every element inside."""
    for j, name in enumerate(ma.NAMES):
        if name in affected:
            assert not (masks[j] & ~touched[j]).any(), name
            assert masks[j].sum() >= 0.95 * touched[j].sum(), (name, int(masks[j].sum()), int(touched[j].sum()))
        else:
            assert not masks[j].any(), name


def test_mutation_denominator_from_the_old_accumulator_is_caught():
    # (a wrong user row reaches the item's gradient of the same example, and so G_Q)
    _assert_caught(*_mutation_masks("old_G"), affected=("P", "Q", "b_u", "b_i", "G_Q"))


def test_mutation_eps_inside_the_root_is_caught():
    """At eps = 1e-10 and G of order one the two placements differ by 5e-11 of the step, below the
    tolerance; the mutation is run at eps = 1e-3, where they differ by 5e-4 of it."""
    _assert_caught(*_mutation_masks("eps_in_root", eps=1e-3), affected=("P", "Q", "b_u", "b_i", "G_Q"))


def test_mutation_item_gradient_from_the_old_user_row_is_caught():
    _assert_caught(*_mutation_masks("stale_user_row"), affected=("Q", "G_Q"))


def test_mutation_one_accumulator_per_row_is_caught():
    _assert_caught(*_mutation_masks("row_acc"), affected=("P", "Q", "G_P", "G_Q"))


# --------------------------------------------------------------------------
# the kinds of the ABI, the geometry query and the argument checks that need no device
# --------------------------------------------------------------------------
def test_optimizer_kinds_and_entry_extend_the_existing_ones():
    """``RFM_MF_OPT_*`` of include/rfm_hip.h are defined as ``RFM_FM_OPT_*``, the Python pair, and the entry is
    rfm_mf_sgd_levels_ex's arguments, unmoved, then kind, four accumulators, eps (the declarations:
    test_host_abi.py)."""
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "rfm_hip.h")).read()
    defines = dict(re.findall(r"#define (RFM_MF_OPT_\w+) (\w+)", header))
    assert defines == {"RFM_MF_OPT_SGD": "RFM_FM_OPT_SGD", "RFM_MF_OPT_ADAGRAD": "RFM_FM_OPT_ADAGRAD"}
    assert (_lib.OPT_SGD, _lib.OPT_ADAGRAD) == (ma.SGD, ma.ADAGRAD)
    ex = _lib.SIGNATURES["rfm_mf_sgd_levels_ex"]
    assert _lib.SIGNATURES["rfm_mf_sgd_levels_opt"][: len(ex)] == ex and len(ex) == 15


@pytest.mark.parametrize("k", ms.SHAPE_KS)
def test_geometry_of_every_class(k):
    case = ms.Case("geometry", k, np.zeros(1, np.int64), np.zeros(1, np.int64), {})
    sgd, ada = ma.assert_class(case, ma.SGD), ma.assert_class(case, ma.ADAGRAD)
    assert ada["lds_bytes_per_cached_item"] == 2 * sgd["lds_bytes_per_cached_item"]
    # the same rows in the cache under both rules: at most 64 KiB instead of 32
    assert ms.capacity(k) * ada["lds_bytes_per_cached_item"] <= 64 << 10
    assert sgd["row_ahead"] == (ms.READ_AHEAD if sgd["chunks_per_lane"] <= 4 else 0)


def test_bad_arguments_that_need_no_device():
    lib = _lib.load()
    out = np.zeros(7, dtype=np.int32)
    for kind in (-1, 2):
        assert lib.rfm_mf_opt_geometry(None, kind, 16, out.ctypes.data) == _lib.RFM_ERR_BAD_ARG
    for k in (0, ms.MAX_FACTORS + 1):
        assert lib.rfm_mf_opt_geometry(None, ma.ADAGRAD, k, out.ctypes.data) == _lib.RFM_ERR_BAD_ARG
    assert lib.rfm_mf_opt_geometry(None, ma.ADAGRAD, 16, None) == _lib.RFM_ERR_BAD_ARG
    # the rule's own checks come before anything is read or launched: host memory stands in for
    # the device arrays, the context is null
    a = np.zeros(64)
    lptr = np.zeros(2, dtype=np.int32)
    ptr = a.ctypes.data

    def call(kind, accs, eps):
        return lib.rfm_mf_sgd_levels_opt(None, ptr, lptr.ctypes.data, ptr, 0, None, 0, ptr, ptr, ptr, ptr, 0.0, 16,
                                         0.1, 0.5, kind, *accs, eps)
    full = (ptr, ptr, ptr, ptr)
    for kind in (-1, 2, 7):
        assert call(kind, full, 1e-10) == _lib.RFM_ERR_BAD_ARG and "neither" in _lib.last_error()
    for j in range(4):
        assert call(ma.ADAGRAD, full[:j] + (None,) + full[j + 1:], 1e-10) == _lib.RFM_ERR_BAD_ARG
        assert "null accumulator" in _lib.last_error()
    for eps in (0.0, -1e-10, float("nan")):
        assert call(ma.ADAGRAD, full, eps) == _lib.RFM_ERR_BAD_ARG and "eps" in _lib.last_error()
    assert call(ma.ADAGRAD, full, 1e-10) == _lib.RFM_ERR_BAD_ARG and "null pointer" in _lib.last_error()  # (the null ctx)


def test_python_checks_that_need_no_launch():
    """The attribute's checks come before any launch (``optimizer.take_optimizer``, as ``fit`` calls it)."""
    from relevance_factorizationmachine_amd.mf import LogisticMatrixFactorization as MF
    from relevance_factorizationmachine_amd.optimizer import take_optimizer

    def take(model):
        return take_optimizer(model, ("P", "Q", "b_u", "b_i"), inexact=model.hogwild)

    class Probe:
        optimizer, adagrad_eps, adagrad_init, hogwild = "sgd", 1e-10, 0.0, False

    assert (MF.optimizer, MF.adagrad_eps, MF.adagrad_init) == ("sgd", 1e-10, 0.0)
    probe = Probe()
    assert take(probe) is False
    probe.optimizer = "adam"
    with pytest.raises(ValueError, match="optimizer must be"):
        take(probe)
    probe.optimizer, probe.adagrad_eps = "adagrad", 0.0
    with pytest.raises(ValueError, match="adagrad_eps"):
        take(probe)
    probe.adagrad_eps, probe.hogwild = 1e-10, True
    with pytest.raises(ValueError, match="exact mode only"):
        take(probe)
