"""The AdaGrad rule of the FM fit on the device (rfm_fm_plan_set_optimizer), through
the raw ABI on grad_forms_common's DeviceLog / Params and through fit().  Needs an MI355X:
``pytest -m gpu``.

One step is held to the long-double oracle element by element, parameters and accumulators alike,
by the intervals of adagrad_common.py (derived there; test_adagrad_host.py shows on every case list
used here that they cannot hide a wrong rule); columns no batch row holds keep their bits.  Where
every sum of a step has a fixed order the step is, bit for bit, the NumPy float64 formula applied
to the plan's own rfm_fm_grad output."""
import numpy as np
import pytest

import adagrad_common as ac
import grad_forms_common as gf
from conftest import assert_elementwise, rel_err
from oracle import cpu_ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from relevance_factorizationmachine_amd import runtime
    return runtime.Runtime.get()


@pytest.fixture(scope="module", autouse=True)
def _leave_no_caches(rt):
    """The fits below would leave their split, plan and sampled ids remembered (30 iterations of the
    coat shape at batch 500): the modules that run after this one start as they did before it."""
    yield
    rt.clear_caches()


def _ids(cases):
    return [f"{gf.class_id(k)}-hot{hot}" for k, hot in cases]


def _one_step(rt, dev, log, theta, G, ids, oracle, what, lr=ac.LR, cold=True):
    params, accs = gf.Params(rt, *theta), gf.Params(rt, *G)
    got_t, got_G = ac.adagrad_step(dev, ids, params, accs, lr)
    ac.assert_inside(got_t, got_G, theta, G, oracle, lr, ac.EPS, len(ids), what)
    ac.assert_untouched_bitwise(got_t, got_G, theta, G, log["features"], ids, what, some=cold)
    return got_t, got_G


# --------------------------------------------------------------------------
# 1. one step at every (lanes per row, vector, chunks) class x hot mode
# --------------------------------------------------------------------------
@pytest.mark.parametrize("k,hot", ac.CASES_A, ids=_ids(ac.CASES_A))
def test_one_step_at_every_shape_class(rt, k, hot):
    log, theta, ids, oracle = ac.case_a(k)
    dev = gf.DeviceLog(rt, log, k, len(ids["full"]), hot)
    try:
        assert dev.plan.layout()["lanes_per_row"] == gf.CLASS_OF[k][0]
        n_hot = dev.plan.info()["hot_columns"]
        assert (n_hot > 0) == (hot != -1 and not gf.chunked(k)), n_hot
        assert ac.optimizer_of(dev) == ac.SGD  # a new plan's rule
        if n_hot:  # the shard leaves hot columns without an entry: visited, and bitwise unchanged
            assert len(np.setdiff1d(dev.plan.hot_columns(), np.unique(log["features"][ids["shard"]].indices))) > 0
        for batch in ("full", "shard"):
            for kind in ac.ACC_KINDS:
                G = ac.acc_init(kind, *theta[2].shape, k)
                got_t, _ = _one_step(rt, dev, log, theta, G, ids[batch], oracle[batch], f"{batch} {kind}")
                assert not np.array_equal(got_t[2], theta[2])
    finally:
        dev.close()


# --------------------------------------------------------------------------
# 2. split columns of both forms (both finalize kernels), and the hot-class overflow
# --------------------------------------------------------------------------
@pytest.mark.parametrize("k,hot,form", ac.CASES_SPLIT, ids=[f"{gf.class_id(k)}-hot{h}-{f}" for k, h, f in ac.CASES_SPLIT])
def test_split_columns(rt, k, hot, form):
    log, theta, full, oracle = ac.case_split(k, form)
    dev = gf.DeviceLog(rt, log, k, len(full), hot)
    try:
        assert dev.geometry()["BC"] == gf.full_batch_workgroup_slots(k)
        parts = dev.partial_rows(0)
        assert (2 <= parts <= ac.K_SHORT_SPLIT) if form == "short" else parts > ac.K_SHORT_SPLIT, parts
        info = dev.plan.info()
        assert info["split_columns"] >= 1 and info["hot_columns"] == 0
        for kind in ac.ACC_KINDS:
            G = ac.acc_init(kind, *theta[2].shape, k)
            # (the full batch of a random log at 5 % density: every column is held by some row)
            got_t, got_G = _one_step(rt, dev, log, theta, G, full, oracle, f"{form} {kind}", cold=False)
            # the split column's row went through the finalize launch
            assert not np.array_equal(got_t[2][0], theta[2][0]) and not np.array_equal(got_G[2][0], G[2][0])
    finally:
        dev.close()


def test_hot_class_overflow_leaves_dense_columns_split(rt):
    log, theta, full, oracle, hot_cap, dense = ac.case_overflow()
    dev = gf.DeviceLog(rt, log, ac.K_OVERFLOW, len(full), 0)
    try:
        info = dev.plan.info()
        assert info["hot_columns"] == hot_cap and info["split_columns"] == dense - hot_cap
        assert 2 <= dev.partial_rows(dense - 1) <= ac.K_SHORT_SPLIT
        for kind in ac.ACC_KINDS:
            _one_step(rt, dev, log, theta, ac.acc_init(kind, *theta[2].shape, ac.K_OVERFLOW), full, oracle, kind,
                      cold=False)
    finally:
        dev.close()


# --------------------------------------------------------------------------
# 3. fixed-order modes: the same bits twice, and the NumPy formula on the plan's own gradient
# --------------------------------------------------------------------------
@pytest.mark.parametrize("k,hot", ac.CASES_FIXED, ids=_ids(ac.CASES_FIXED))
def test_fixed_order_step_is_the_float64_formula_on_the_plans_gradient(rt, k, hot):
    log, theta, ids, _ = ac.case_a(k)
    n = theta[1].shape[0]
    dev = gf.DeviceLog(rt, log, k, len(ids["full"]), hot)
    try:
        assert gf.fixed_order(k, hot)
        for batch in ("full", "shard"):
            G = ac.acc_init("uniform", n, k, k)
            g, _ = gf.dense_grad(dev, ids[batch], gf.Params(rt, *theta))
            G_V, g_w, g_w0 = gf.split_grad(g, n, k)
            want = [ac.rule_f64(t, a, gg, ac.LR, ac.EPS) for t, a, gg in zip(theta, G, (np.array([g_w0]), g_w, G_V))]
            runs = [ac.adagrad_step(dev, ids[batch], gf.Params(rt, *theta), gf.Params(rt, *G)) for _ in range(2)]
            for i, name in enumerate(("w0", "w", "V")):
                for j, part in enumerate(("parameter", "accumulator")):
                    assert np.array_equal(runs[0][j][i], runs[1][j][i]), f"{batch} {name} {part}: two runs differ"
                    assert np.array_equal(runs[0][j][i], want[i][j]), f"{batch} {name} {part}: not the float64 formula"
    finally:
        dev.close()


# --------------------------------------------------------------------------
# 4. three steps on one plan (both parities of the chunked bitmap)
# --------------------------------------------------------------------------
@pytest.mark.parametrize("k", ac.KS_THREE_STEPS)
def test_three_steps_on_one_plan(rt, k):
    log = ac.log_a(False)
    n = log["features"].shape[1]
    theta = gf.perturbed_init(k, n, k)
    G = ac.acc_init("zero", n, k, k)
    dev = gf.DeviceLog(rt, log, k, ac.THREE_BATCH, 0)
    try:
        assert gf.chunked(k) and dev.plan.info()["hot_columns"] == 0
        params, accs = gf.Params(rt, *theta), gf.Params(rt, *G)
        for step, ids in enumerate(ac.three_batches(k)):
            oracle = gf.grad_oracle(log, ids, *theta)  # from the device's own previous state
            got_t, got_G = ac.adagrad_step(dev, ids, params, accs)
            ac.assert_inside(got_t, got_G, theta, G, oracle, ac.LR, ac.EPS, len(ids), f"step {step}")
            ac.assert_untouched_bitwise(got_t, got_G, theta, G, log["features"], ids, f"step {step}")
            theta, G = got_t, got_G
    finally:
        dev.close()


# --------------------------------------------------------------------------
# 5. edges
# --------------------------------------------------------------------------
@pytest.mark.parametrize("hot", [0, -1])
def test_edges(rt, hot):
    k = 16
    log, theta, ids, _ = ac.case_a(k)
    n = theta[1].shape[0]
    X = log["features"]
    dev = gf.DeviceLog(rt, log, k, len(ids["full"]), hot)
    try:
        G = ac.acc_init("uniform", n, k, k)
        # a batch of one row; a batch of one EMPTY row (w0 alone moves)
        one, empty = np.array([11], dtype=np.int32), np.array([5], dtype=np.int32)
        assert X[11].nnz > 0 and X[5].nnz == 0
        _one_step(rt, dev, log, theta, G, one, gf.grad_oracle(log, one, *theta), "one row")
        params, accs = gf.Params(rt, *theta), gf.Params(rt, *G)
        got_t, got_G = ac.adagrad_step(dev, empty, params, accs)
        ac.assert_inside(got_t, got_G, theta, G, gf.grad_oracle(log, empty, *theta), ac.LR, ac.EPS, 1, "empty row")
        assert got_t[0][0] != theta[0][0] and got_G[0][0] > G[0][0]
        for i in (1, 2):
            assert np.array_equal(got_t[i], theta[i]) and np.array_equal(got_G[i], G[i])
        # lr = 0: parameters bitwise unchanged, accumulators grow
        got_t, got_G = _one_step(rt, dev, log, theta, G, ids["full"], gf.grad_oracle(log, ids["full"], *theta),
                                 "lr = 0", lr=0.0)
        touched = np.unique(X[ids["full"]].indices)
        for i in range(3):
            assert np.array_equal(got_t[i], theta[i])
        assert got_G[0][0] > G[0][0] and (got_G[1][touched] >= G[1][touched]).all()
        assert (got_G[2][touched] >= G[2][touched]).all()
        # (a gradient below 1e-8 adds nothing to an accumulator of order one: nearly all grow)
        assert (got_G[1][touched] > G[1][touched]).mean() > 0.9 and (got_G[2][touched] > G[2][touched]).mean() > 0.9
        # accumulators at +Inf (a column of the sparse class, and a hot one where there is a hot class):
        # those columns' parameters keep their bits, the others move
        hot_cols = dev.plan.hot_columns()
        cols = [int(np.setdiff1d(touched, hot_cols)[0])] + ([int(hot_cols[0])] if len(hot_cols) else [])
        G_inf = [a.copy() for a in G]
        G_inf[1][cols], G_inf[2][cols] = np.inf, np.inf
        params, accs = gf.Params(rt, *theta), gf.Params(rt, *G_inf)
        got_t, got_G = ac.adagrad_step(dev, ids["full"], params, accs)
        assert np.array_equal(got_t[1][cols], theta[1][cols]) and np.array_equal(got_t[2][cols], theta[2][cols])
        assert np.isposinf(got_G[1][cols]).all() and np.isposinf(got_G[2][cols]).all()
        rest = np.setdiff1d(touched, cols)
        assert (got_t[1][rest] != theta[1][rest]).mean() > 0.9 and not np.isnan(got_t[2]).any()
    finally:
        dev.close()


# --------------------------------------------------------------------------
# 6. the rule is the plan's: AdaGrad, then SGD again; bad arguments
# --------------------------------------------------------------------------
@pytest.mark.parametrize("k", [16, 65])
def test_reset_to_sgd_is_the_fresh_plans_sgd_step(rt, k):
    import torch

    log, theta, ids, _ = ac.case_a(k)
    n = theta[1].shape[0]
    lr = 1e-3
    dev = gf.DeviceLog(rt, log, k, len(ids["full"]), -1)
    fresh = gf.DeviceLog(rt, log, k, len(ids["full"]), -1)
    try:
        # the accumulators between NaN sentinels in ONE buffer
        pad = 8
        sizes = (1, n, n * k)
        buf = torch.full((sum(sizes) + pad * 4,), float("nan"), dtype=torch.float64, device=rt.torch_device)
        views, at = [], pad
        for s in sizes:
            views.append(buf[at: at + s])
            at += s + pad

        class Accs:
            def ptrs(self):
                return tuple(v.data_ptr() for v in views)

        for v in views:
            v.fill_(0.5)
        params = gf.Params(rt, *theta)
        from relevance_factorizationmachine_amd import _lib
        _lib.check(ac.set_optimizer(dev, ac.ADAGRAD, Accs()))
        assert ac.optimizer_of(dev) == ac.ADAGRAD
        gf.step(dev, ids["full"], params, ac.LR)
        theta1 = [a.copy() for a in params.host()]
        after_ada = buf.cpu().numpy().copy()
        assert (after_ada[pad: pad + 1] > 0.5).all() and not np.array_equal(theta1[2], theta[2])
        _lib.check(ac.set_optimizer(dev, ac.SGD))
        assert ac.optimizer_of(dev) == ac.SGD
        gf.step(dev, ids["shard"], params, lr)
        gf.step(dev, ids["full"], params, lr)
        ref = gf.Params(rt, *theta1)
        gf.step(fresh, ids["shard"], ref, lr)
        gf.step(fresh, ids["full"], ref, lr)
        for a, b in zip(params.host(), ref.host()):
            assert np.array_equal(a, b)
        now = buf.cpu().numpy()
        assert np.array_equal(now, after_ada, equal_nan=True), "an SGD step wrote an accumulator"
        guards = np.ones(now.shape, bool)
        at = pad
        for s in sizes:
            guards[at: at + s] = False
            at += s + pad
        assert np.isnan(now[guards]).all() and not np.isnan(now[~guards]).any()
    finally:
        dev.close()
        fresh.close()


def test_bad_arguments(rt):
    from relevance_factorizationmachine_amd import _lib
    log, theta, ids, _ = ac.case_a(16)
    dev = gf.DeviceLog(rt, log, 16, 64, 0)
    try:
        accs = gf.Params(rt, *ac.acc_init("zero", *theta[2].shape, 16))
        a0, aw, aV = accs.ptrs()
        lib, h = rt.lib, dev.plan.handle
        for args in ((1, None, aw, aV, 1e-10), (1, a0, None, aV, 1e-10), (1, a0, aw, None, 1e-10),
                     (1, a0, aw, aV, 0.0), (1, a0, aw, aV, -1.0), (1, a0, aw, aV, float("nan")), (2, a0, aw, aV, 1e-10),
                     (-1, None, None, None, 0.0)):
            assert lib.rfm_fm_plan_set_optimizer(h, *args) == _lib.RFM_ERR_BAD_ARG, args
            assert ac.optimizer_of(dev) == ac.SGD
        _lib.check(ac.set_optimizer(dev, ac.ADAGRAD, accs))
        assert lib.rfm_fm_plan_set_optimizer(h, 1, a0, aw, aV, 0.0) == _lib.RFM_ERR_BAD_ARG
        assert ac.optimizer_of(dev) == ac.ADAGRAD  # a refused call leaves the rule
        # the data-parallel fit refuses the plan before anything else
        params = gf.Params(rt, *theta)
        d_ids = rt.upload(np.arange(64, dtype=np.int32))
        tl = rt.upload(np.zeros(1))
        args = (rt.ctx, h, None, 0, d_ids.data_ptr(), 64, 1, *params.ptrs(), 1e-3, None, None, None, None, None, 0, 1e-8,
                tl.data_ptr(), None)
        assert lib.rfm_fm_fit_dp(*args) == _lib.RFM_ERR_BAD_ARG
        assert "SGD" in _lib.last_error()
        for a, b in zip(params.host(), theta):
            assert np.array_equal(a, np.asarray(b).reshape(a.shape))
        # gradient mode ignores the rule: the same bits as under SGD
        g_ada, _ = gf.dense_grad(dev, ids["shard"], params)
        _lib.check(ac.set_optimizer(dev, ac.SGD))
        g_sgd, _ = gf.dense_grad(dev, ids["shard"], params)
        assert np.array_equal(g_ada, g_sgd)
    finally:
        dev.close()


# --------------------------------------------------------------------------
# 7. through Python
# --------------------------------------------------------------------------
def _model(est, g, **kw):
    import relevance_factorizationmachine_amd as pkg
    train, val = ac.coat_split(est)
    args = dict(estimator=est, n_epochs=int(g["n_epochs"]), n_factors=8, n_features=train["features"].shape[1],
                lr=float(g["lr"]), batch_size=500, seed=int(g["seed"]))
    args.update(kw)
    m = pkg.FactorizationMachines(**args)
    m.optimizer, m.adagrad_eps, m.adagrad_init = "adagrad", float(g["eps"]), float(g["init"])
    return m, train, val


def _state(m):
    return [m.w0(), m.w(), m.V(), m.w0.acc.cpu().numpy(), m.w.acc.cpu().numpy(), m.V.acc.cpu().numpy()]


@pytest.mark.parametrize("est", ["IPS", "Naive"])
def test_fit_against_the_reference_with_an_adagrad_subclass(golden, est):
    import relevance_factorizationmachine_amd as pkg
    g = golden("fm_adagrad_coat_k8")
    m, train, val = _model(est, g)
    tr, va = m.fit(train, val)
    assert isinstance(m.V, pkg.DeviceAdaGrad) and isinstance(m.w0, pkg.DeviceAdaGrad)
    got = dict(zip(("w0", "w", "V", "acc_w0", "acc_w", "acc_V"), _state(m)), train_loss=tr, val_loss=va)
    for name, have in got.items():
        want = g[f"{est}_{name}"]
        print(f"{est} {name}: rel_err {rel_err(have, want):.3g}")
        assert rel_err(have, want) < 1e-9, name
        assert_elementwise(have, want, what=f"{est} {name}")


def test_fit_deterministic_twice_and_with_an_evaluator(golden):
    """deterministic = True: two fits give the same bits, and a fit with a ValEvaluator (rfm_fm_train_eval)
    leaves the parameters of the fit without one (rfm_fm_train): both take the plan's rule."""
    from relevance_factorizationmachine_amd import synth
    from test_gpu_eval import _ValEvaluatorLike
    g = golden("fm_adagrad_coat_k8")
    states = []
    for with_ev in (False, False, True):
        ev = None
        if with_ev:
            _, val_mf = synth.make_log(synth.SHAPES["coat"], "MF", "IPS", seed=0)
            _, val = ac.coat_split("IPS")
            ev = _ValEvaluatorLike(synth.interaction_frame(val_mf, val_mf["features"]), {"FM": val["features"]})
        m, train, val = _model("IPS", g, n_epochs=9, evaluator=ev)
        m.deterministic = True
        m.fit(train, val)
        if with_ev:
            assert len(m.val_metrics) == 9
        states.append(_state(m))
    for a, b, c in zip(*states):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    assert (states[0][5] > 0).any()


def test_accumulators_persist_append_columns_and_errors(golden):
    import torch
    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import dist
    from relevance_factorizationmachine_amd.fm import FoldedColumns
    g = golden("fm_adagrad_coat_k8")
    m, train, val = _model("IPS", g, n_epochs=2)
    m.adagrad_init = 0.25
    m.fit(train, val)
    acc1 = m.V.acc.cpu().numpy().copy()
    assert acc1.min() >= 0.25 and acc1.max() > 0.25
    m.fit(train, val)  # the same handles, the accumulators go on growing
    acc2 = m.V.acc.cpu().numpy()
    assert (acc2 >= acc1).all() and (acc2 > acc1).any()
    rt, n = m._rt, m.n_features
    folded = FoldedColumns("user", torch.ones(3, dtype=torch.float64, device=rt.torch_device),
                           torch.ones((3, 8), dtype=torch.float64, device=rt.torch_device), None, None, rt)
    assert list(m.append_columns(folded)) == [n, n + 1, n + 2]
    assert tuple(m.V.acc.shape) == (n + 3, 8) and tuple(m.w.acc.shape) == (n + 3,) and tuple(m.V.dev.shape) == (n + 3, 8)
    assert np.array_equal(m.V.acc.cpu().numpy()[n:], np.full((3, 8), 0.25)) and np.array_equal(m.V.acc.cpu().numpy()[:n], acc2)
    assert np.array_equal(m.w.acc.cpu().numpy()[n:], np.full(3, 0.25))
    # a shared plan goes back to the cache with the SGD rule: an SGD model on the same split is the parent's
    s1 = pkg.FactorizationMachines(estimator="IPS", n_epochs=3, n_factors=8, n_features=n, lr=1e-4, batch_size=500, seed=1)
    s1.deterministic = True
    s1.fit(train, val)
    assert type(s1.V) is pkg.DeviceSGD
    bad, _, _ = _model("IPS", g, n_epochs=2)
    bad.optimizer = "adam"
    with pytest.raises(ValueError, match="optimizer"):
        bad.fit(train, val)
    m2, _, _ = _model("IPS", g, n_epochs=2)
    before = m2.V()
    with pytest.raises(ValueError, match="SGD rule only"):
        dist.fit_data_parallel(m2, train, val)
    assert np.array_equal(m2.V(), before)
