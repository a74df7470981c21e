"""Several MF models on one schedule -- rfm_mf_sgd_levels_many, rfm_mf_predict_many,
rfm_mf_predict_loss_many through the raw C ABI, and mf.fit_many on top of them.  Needs an MI355X:
``pytest -m gpu``.

A step test runs M models that differ in everything they may differ in (mf_many_common.py) on the
shared schedule of a case of mf_step_common.py and asserts, per model: (i) its P, Q, b_u, b_i equal BIT
FOR BIT what rfm_mf_sgd_levels_ex gives on that model's own records alone; (ii) they lie within
``ms.MF_TOL`` of the long-double oracle for that model; (iii) two calls from the same start give the
same bits.  Every array sits between sentinels and rows outside the batch keep their bits.
test_mf_many_host.py shows on the CPU that these cases at this tolerance see a neighbour's labels, a
cache written back into another model and a dropped record-to-row indirection.

The scoring calls are held, bit for bit, to rfm_mf_predict / rfm_mf_predict_loss on each model alone;
fit_many to each model's own fit() in the same process."""
import numpy as np
import pytest

import mf_many_common as mm
import mf_step_common as ms
from conftest import assert_elementwise, load_golden, rel_err
from relevance_factorizationmachine_amd import synth

pytestmark = pytest.mark.gpu

NAMES = ("P", "Q", "b_u", "b_i")


@pytest.fixture(scope="module")
def rt():
    from relevance_factorizationmachine_amd import runtime
    return runtime.Runtime.get()


def _n_cu(rt):
    import torch
    return int(torch.cuda.get_device_properties(rt.device).multi_processor_count)


def _check_many(rt, case, n_models):
    sched = mm.reach_rows(case)  # asserts the launches and record states the case is named for
    assert not np.array_equal(sched[1], np.arange(len(sched[1])))  # ex_rows is not the identity
    models = mm.models_of(case, n_models)
    first = mm.run_levels_many(rt, case, sched, models)
    second = mm.run_levels_many(rt, case, sched, models)
    worst = 0.0
    for mod, got, again in zip(models, first, second):
        what = f"{case.name} model {mod.m} of {n_models}"
        alone = mm.run_levels_alone(rt, case, sched, mod)
        for nm, a, b, c in zip(NAMES, got, alone, again):
            np.testing.assert_array_equal(a, b, err_msg=f"{what}: {nm} differs from rfm_mf_sgd_levels_ex alone")  # (i)
            np.testing.assert_array_equal(a, c, err_msg=f"{what}: {nm} of two calls from the same start differ")  # (iii)
        worst = max(worst, ms.assert_params_within(got, mm.oracle_of(case, mod), mod.init, case.pairs, ms.MF_TOL, what))  # (ii)
    print(f"distance {case.name} M={n_models} {worst:.3e}")


# every shape class at its lowest factor count: a wide level, then a sequential run
@pytest.mark.parametrize("k", [lo for lo, _ in ms.CLASS_RANGE.values()])
def test_every_shape_class(rt, k):
    case = ms.step_cases()[f"shape-k{k}"]
    assert [p[0] for p in case.want_plan["levels_ex"]] == ["wide", "seq"]
    geo = mm.geometry_py(3, k, case.want_plan["levels_ex"][0][2], _n_cu(rt))
    from relevance_factorizationmachine_amd.runtime import mf_many_geometry
    assert mf_many_geometry(rt, 3, k, case.want_plan["levels_ex"][0][2]) == geo and geo["wide_grid_y"] == 3
    _check_many(rt, case, 3)


@pytest.mark.parametrize("name", ["ring-cached-k16", "ring-uncached-k16", "ring-fresh-k16", "ring-full-k300",
                                  "ring-start-k16"])
def test_read_ahead_ring(rt, name):
    _check_many(rt, ms.step_cases()[name], 3)


# two sequential launches per call; the item cache at and beyond capacity (the raised LDS limit, each
# model's own write-back); seq -> wide -> seq
@pytest.mark.parametrize("name", ["limit-levels1029-k16", "limit-recs1025-k300", "limit-cache-k400", "limit-cache-k3",
                                  "limit-grow-k300"])
def test_launch_limits(rt, name):
    case = ms.step_cases()[name]
    if name.startswith(("limit-levels", "limit-recs")):
        assert [p[0] for p in case.want_plan["levels_ex"]] == ["seq", "seq"]
    _check_many(rt, case, 2)


def test_one_model(rt):
    _check_many(rt, ms.step_cases()["ring-cached-k16"], 1)


def test_more_sequential_workgroups_than_cus(rt):
    from relevance_factorizationmachine_amd.runtime import mf_many_geometry
    n_models = _n_cu(rt) + 1
    geo = mf_many_geometry(rt, n_models, 16, 0)
    assert geo["seq_grid"] == n_models > _n_cu(rt) and geo["seq_threads"] == ms.SEQ_BLOCK
    _check_many(rt, ms.step_cases()["ring-cached-k16"], n_models)


def test_wide_level_past_one_pass_of_the_grid(rt):
    from relevance_factorizationmachine_amd.runtime import mf_many_geometry
    n_cu = _n_cu(rt)
    case = ms.grid_case(2, n_cu)
    geo = mf_many_geometry(rt, 2, 2, len(case.users))
    assert geo["wide_grid_x"] == n_cu * ms.GRID_PER_CU and geo["wide_grid_y"] == 2
    assert len(case.users) > ms.grid_pass(2, n_cu)
    _check_many(rt, case, 2)


def test_step_rejects_bad_arguments(rt):
    from relevance_factorizationmachine_amd import _lib
    case = ms.step_cases()["ring-cached-k16"]
    ex, ex_rows, lptr, cache = mm.reach_rows(case)
    models = mm.models_of(case, 1)
    table = mm.ModelTable(rt, models, [models[0].ry_log])
    d_ex, d_rows, d_lptr, d_cache = (rt.upload(a) for a in (np.ascontiguousarray(ex).view(np.uint8), ex_rows, lptr, cache))

    def call(ex_ptr=d_ex.data_ptr(), rows_ptr=d_rows.data_ptr(), models_ptr=table.ptr, n_models=1, n_cached=len(cache)):
        return rt.lib.rfm_mf_sgd_levels_many(rt.ctx, ex_ptr, rows_ptr, lptr.ctypes.data, d_lptr.data_ptr(), len(lptr) - 1,
                                             d_cache.data_ptr(), n_cached, models_ptr, n_models, case.k)

    for kw in (dict(n_models=0), dict(n_models=1025), dict(ex_ptr=None), dict(rows_ptr=None), dict(models_ptr=None),
               dict(n_cached=ms.capacity(case.k) + 1)):
        assert call(**kw) == _lib.RFM_ERR_BAD_ARG, kw
    for got, start in zip(table.host()[0], models[0].init):  # nothing ran
        np.testing.assert_array_equal(got, start)


# --------------------------------------------------------------------------
# rfm_mf_predict_many / rfm_mf_predict_loss_many
# --------------------------------------------------------------------------
@pytest.mark.parametrize("with_ids", [False, True])
@pytest.mark.parametrize("k", [2, 128, 400])
def test_scores_and_losses_equal_each_model_alone(rt, k, with_ids):
    from relevance_factorizationmachine_amd.runtime import mf_many_geometry
    sizes = ms.predict_sizes(k, _n_cu(rt))
    for n_rows in sorted(set(sizes[:2] + sizes[-1:])):
        prob = ms.predict_problem(k, n_rows, with_ids)
        models, labels = mm.predict_models(prob, 3)
        geo = mf_many_geometry(rt, 3, k, n_rows)
        assert geo["predict_grid_y"] == 3 and geo == mm.geometry_py(3, k, n_rows, _n_cu(rt))
        scores, _ = mm.run_predict_many(rt, prob, models, labels, loss=False)
        fused, losses = mm.run_predict_many(rt, prob, models, labels, loss=True)
        for mod, lab, s, f, lo in zip(models, labels, scores, fused, losses):
            what = f"k={k} n={n_rows} ids={with_ids} model {mod.m}"
            alone, _ = mm.predict_alone(rt, prob, mod, lab, loss=False)
            alone_fused, alone_loss = mm.predict_alone(rt, prob, mod, lab, loss=True)
            np.testing.assert_array_equal(s, alone, err_msg=what)
            np.testing.assert_array_equal(f, alone_fused, err_msg=what)
            assert np.float64(lo).tobytes() == np.float64(alone_loss).tobytes(), (what, lo, alone_loss)


# --------------------------------------------------------------------------
# fit_many on the small MF log of the parity tests
# --------------------------------------------------------------------------
FIXTURE = dict(n_epochs=3, n_factors=16, lr=0.01, reg=0.5, batch_size=2000, seed=12345)  # test_gpu_parity.py


@pytest.fixture(scope="module")
def small():
    sh = synth.SHAPES["kuairec_small"]
    logs = {est: synth.make_log(sh, "MF", est, seed=0) for est in ("IPS", "Naive")}
    # the synthetic Naive log draws other validation rows; a loader gives both estimators the same rows
    # and propensities of one under Naive: the IPS validation rows at propensity 1
    train, val = logs["Naive"][0], logs["IPS"][1]
    np.testing.assert_array_equal(train["features"], logs["IPS"][0]["features"])
    assert (train["pscores"] == 1.0).all()
    logs["Naive"] = (train, dict(val, pscores=np.ones_like(val["pscores"])))
    return sh, logs


def _five(sh, logs, with_evaluator=True, **override):
    """IPS and Naive at the fixture's settings, then seed + 1, lr x 0.5 and reg x 2: (models, trains, vals)."""
    import relevance_factorizationmachine_amd as pkg
    variants = [("IPS", {}), ("Naive", {}), ("IPS", {"seed": FIXTURE["seed"] + 1}), ("IPS", {"lr": FIXTURE["lr"] * 0.5}),
                ("IPS", {"reg": FIXTURE["reg"] * 2})]
    models, trains, vals = [], [], []
    for est, change in variants:
        train, val = logs[est]
        kw = dict(FIXTURE, estimator=est, n_users=sh.n_users, n_items=sh.n_items)
        kw.update(change)
        kw.update(override)
        if with_evaluator:
            kw["evaluator"] = mm.ValEvaluatorLike(synth.interaction_frame(val, val["features"]), {"MF": val["features"]})
        models.append(pkg.LogisticMatrixFactorization(**kw))
        trains.append(train)
        vals.append(val)
    return models, trains, vals


def _assert_same_model(a, b, what):
    for nm in NAMES:
        np.testing.assert_array_equal(getattr(a, nm)(), getattr(b, nm)(), err_msg=f"{what} {nm}")
    assert a.b == b.b
    if a.evaluator is not None:
        assert a.val_metrics == b.val_metrics and len(a.val_metrics) == a.n_epochs, what
        assert a.evaluator_host_calls == b.evaluator_host_calls and a.evaluator_host_users == b.evaluator_host_users
        assert a.evaluator.calls == 0  # the evaluator object is never called


def _assert_same_losses(got, want, what):
    for g, w, nm in zip(got, want, ("train_loss", "val_loss")):
        assert isinstance(g, list) and len(g) == len(w), what
        np.testing.assert_array_equal(np.asarray(g), np.asarray(w), err_msg=f"{what} {nm}")


def test_fit_many_equals_every_models_own_fit(small):
    from relevance_factorizationmachine_amd import mf
    sh, logs = small
    many, trains, vals = _five(sh, logs)
    alone, _, _ = _five(sh, logs)
    losses = mf.fit_many(many, trains, vals)
    assert len(losses) == 5
    for j, (a, b, t, v) in enumerate(zip(many, alone, trains, vals)):
        want = b.fit(t, v)
        _assert_same_losses(losses[j], want, f"model {j}")
        _assert_same_model(a, b, f"model {j}")
    # the IPS model at the fixture's settings against the reference's golden, as the parity tests hold it
    g = load_golden("mf_small")
    model, (tr, va) = many[0], losses[0]
    pred = model.predict(vals[0]["features"])
    for got, name in ((model.P(), "P"), (model.Q(), "Q"), (model.b_u(), "b_u"), (model.b_i(), "b_i"),
                      (tr, "train_loss"), (va, "val_loss"), (pred, "pred_val")):
        assert rel_err(got, g[f"IPS_{name}"]) < 1e-9, name
        assert_elementwise(got, g[f"IPS_{name}"], what=f"mf_small IPS {name}")
    assert model.b == float(g["IPS_b"])


def test_fit_many_shared_dicts_single_model_and_no_epochs(small):
    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import mf
    sh, logs = small
    train, val = logs["IPS"]
    kw = dict(FIXTURE, estimator="IPS", n_users=sh.n_users, n_items=sh.n_items)
    # one dict for all, no evaluator, two models that differ in alpha
    many = [pkg.LogisticMatrixFactorization(**kw), pkg.LogisticMatrixFactorization(alpha=2.0, **kw)]
    alone = [pkg.LogisticMatrixFactorization(**kw), pkg.LogisticMatrixFactorization(alpha=2.0, **kw)]
    losses = mf.fit_many(many, train, val)
    for j, (a, b) in enumerate(zip(many, alone)):
        _assert_same_losses(losses[j], b.fit(train, val), f"shared model {j}")
        _assert_same_model(a, b, f"shared model {j}")
    # a single model
    one, ref = pkg.LogisticMatrixFactorization(**kw), pkg.LogisticMatrixFactorization(**kw)
    got = mf.fit_many([one], [train], [val])
    _assert_same_losses(got[0], ref.fit(train, val), "single")
    _assert_same_model(one, ref, "single")
    # no iterations: the global bias only
    none = [pkg.LogisticMatrixFactorization(**dict(kw, n_epochs=0)) for _ in range(2)]
    start = [m.P() for m in none]
    assert mf.fit_many(none, train, val) == [([], []), ([], [])]
    for m, p in zip(none, start):
        assert m.b == np.mean(train["labels"])
        np.testing.assert_array_equal(m.P(), p)
    assert mf.fit_many([], train, val) == []


def test_fit_many_with_a_validation_split_of_no_rows(small):
    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import mf
    sh, logs = small
    train, _ = logs["IPS"]
    empty = {"features": np.zeros((0, 2), dtype=np.int64), "labels": np.zeros(0), "pscores": np.ones(0)}
    kw = dict(FIXTURE, estimator="IPS", n_users=sh.n_users, n_items=sh.n_items)
    many = [pkg.LogisticMatrixFactorization(**kw), pkg.LogisticMatrixFactorization(**dict(kw, lr=0.02))]
    alone = [pkg.LogisticMatrixFactorization(**kw), pkg.LogisticMatrixFactorization(**dict(kw, lr=0.02))]
    losses = mf.fit_many(many, train, empty)
    for j, (a, b) in enumerate(zip(many, alone)):
        want = b.fit(train, empty)
        assert np.isnan(want[1]).all() and len(want[1]) == FIXTURE["n_epochs"]
        _assert_same_losses(losses[j], want, f"empty val model {j}")
        _assert_same_model(a, b, f"empty val model {j}")


def test_fit_many_names_what_it_refuses(small):
    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import mf
    from relevance_factorizationmachine_amd.evaluate import CatalogueValEvaluator
    sh, logs = small
    train, val = logs["IPS"]
    kw = dict(FIXTURE, estimator="IPS", n_users=sh.n_users, n_items=sh.n_items, n_epochs=1)

    def pair(**change):
        return [pkg.LogisticMatrixFactorization(**kw), pkg.LogisticMatrixFactorization(**dict(kw, **change))]

    for field, value in (("n_users", sh.n_users + 1), ("n_items", sh.n_items + 1), ("n_factors", 8),
                         ("batch_size", 1000), ("n_epochs", 2)):
        with pytest.raises(ValueError, match=field):
            mf.fit_many(pair(**{field: value}), train, val)
    other = dict(train, features=train["features"][::-1].copy())
    with pytest.raises(ValueError, match="train features"):
        mf.fit_many(pair(), [train, other], val)
    other = dict(val, features=val["features"][::-1].copy())
    with pytest.raises(ValueError, match="val features"):
        mf.fit_many(pair(), train, [val, other])
    with pytest.raises(ValueError, match="one per model"):
        mf.fit_many(pair(), [train], val)
    models = pair()
    models[1].hogwild = True
    with pytest.raises(ValueError, match="hogwild"):
        mf.fit_many(models, train, val)

    def evaluator():
        return mm.ValEvaluatorLike(synth.interaction_frame(val, val["features"]), {"MF": val["features"]})

    class HostCallback:  # the right attributes, but an evaluate() nobody vouches for
        k, metric_name = 5, "DCG"

        def __init__(self):
            self.interaction_df, self.features = synth.interaction_frame(val, val["features"]), {"MF": val["features"]}

        def evaluate(self, y_scores, estimator):
            return 0.0

    def with_evaluators(first, second):
        return [pkg.LogisticMatrixFactorization(evaluator=first, **kw), pkg.LogisticMatrixFactorization(evaluator=second, **kw)]

    with pytest.raises(ValueError, match=r"CatalogueValEvaluator.*fit\(\)"):
        mf.fit_many(with_evaluators(evaluator(), object.__new__(CatalogueValEvaluator)), train, val)
    with pytest.raises(ValueError, match=r"host callback.*fit\(\)"):
        mf.fit_many(with_evaluators(evaluator(), HostCallback()), train, val)
    models = with_evaluators(evaluator(), evaluator())
    models[0].device_evaluator = False
    with pytest.raises(ValueError, match=r"device_evaluator.*fit\(\)"):
        mf.fit_many(models, train, val)
    with pytest.raises(ValueError, match="evaluator"):
        mf.fit_many(with_evaluators(evaluator(), None), train, val)
    short = mm.ValEvaluatorLike(synth.interaction_frame({k: v[:100] for k, v in val.items()}, val["features"][:100]),
                                {"MF": val["features"][:100]})
    with pytest.raises(ValueError, match="evaluator features"):
        mf.fit_many(with_evaluators(evaluator(), short), train, val)
