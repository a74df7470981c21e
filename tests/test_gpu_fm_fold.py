"""FM fold-in on the device -- rfm_fm_fold_in through the raw C ABI against the long-double oracle of
fm_fold_common.py, and fold_in_users / fold_in_items / append_columns / new_users= through Python: at
every (lanes per example, vector width, chunks per lane) class of the kernel with rows of 0, 1, GPB-1,
GPB, GPB+1 and 2 GPB+1 examples side by side (GPB = lane groups of a workgroup) and one of 1 029 at the
narrowest classes, under 0..3 passes, at the row counts around the capped grid, with repeated and
shared fixed rows, clipped logits and a caller's init.  Needs an MI355X: ``pytest -m gpu``.

Every case asserts the shape it means from rfm_fm_fold_geometry.  Every call is made twice from the
same start and must give the same bits (no atomics, no sum whose order depends on timing).  Factor
rows are held to the oracle element by element relative to their own row, weights relative to
max(|w|, lr), at ``FMFOLD_TOL`` (derived from a CPU measurement, see fm_fold_common.py), the served
operands A_new, L_new on the same scales; a column without examples, every input and the sentinels
around every array keep their bits.

On the code before FM fold-in every test here fails: the entry points and the methods do not exist."""
import numpy as np
import pytest
import scipy.sparse as sp

import fm_fold_common as fc
import mf_step_common as ms
from conftest import rel_err
from fold_common import _bits, _n_cu, _names, _twice
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

TIGHT = 1e-9  # the norm-wise bound of the parity tests (test_gpu_parity.py), for the fit on the grown model


@pytest.fixture(scope="module")
def rt():
    from relevance_factorizationmachine_amd import runtime
    return runtime.Runtime.get()


def _check(rt, case):
    g = fc.geometry(case.n_new, case.k, rt)
    cls = ms.shape_class(case.k)
    assert (g["lpr"], g["vec"], g["nc"]) == cls and ms.CLASS_RANGE[cls][0] <= case.k <= ms.CLASS_RANGE[cls][1]
    assert g["groups"] == 256 // g["lpr"] and g["grid"] == min(case.n_new, _n_cu(rt) * fc.GRID_PER_CU)
    V, w, A, L = _twice(lambda: fc.run_fold(rt, case))
    want = fc.oracle(case)
    d = fc.assert_within((V, w), want, fc.FMFOLD_TOL, case.name, case.lr)
    d = max(d, fc.assert_within((A, L), fc.served_all(case, *want), fc.FMFOLD_TOL, f"{case.name} operands", case.lr))
    print(f"distance {case.name} {d:.3e}")
    assert not A[:, case.k:].any(), "the padding of A_new is not zero"
    nu0, om0 = case.start()
    idle = np.flatnonzero(case.lengths * case.n_passes == 0)
    np.testing.assert_array_equal(_bits(V[idle]), _bits(nu0[idle]), err_msg="a column without examples changed")
    np.testing.assert_array_equal(_bits(w[idle]), _bits(om0[idle]), err_msg="a weight without examples changed")
    return (V, w, A, L), g


# --------------------------------------------------------------------------
# a. every shape class at its lowest and highest factor count
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("shape-", fc.fold_cases()))
def test_every_shape_class(rt, name):
    case = fc.fold_cases()[name]
    _, g = _check(rt, case)
    gpb = g["groups"]
    assert {0, 1, gpb - 1, gpb, gpb + 1, 2 * gpb + 1} <= set(case.lengths.tolist())
    if g["lpr"] == 4:
        assert fc.LONG_ROW in case.lengths and fc.LONG_ROW % gpb and fc.LONG_ROW > 16 * gpb


# --------------------------------------------------------------------------
# b. 0, 1, 2, 3 passes
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("passes", fc.fold_cases()))
def test_passes(rt, name):
    case = fc.fold_cases()[name]
    got, _ = _check(rt, case)
    if case.n_passes == 0:
        for a, b in zip(got[:2], case.start()):
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg="no passes changed a column")
    if case.n_passes >= 2:
        # only the passes are sequential, so p passes are p calls of one pass, bit for bit
        step = case.start()
        for _ in range(case.n_passes):
            out = fc.run_fold(rt, case, start=step, n_passes=1)
            step = out[:2]
        for a, b in zip(got, out):
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg="one call of p passes and p calls of one differ")


# --------------------------------------------------------------------------
# c. row counts around the capped grid: the grid-stride
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("count", fc.fold_cases()))
def test_row_counts(rt, name):
    case = fc.fold_cases()[name]
    assert fc.geometry(case.n_new, case.k)["grid"] == min(case.n_new, fc.ASSUMED_GRID)
    assert case.n_new in (1, fc.ASSUMED_GRID - 1, fc.ASSUMED_GRID, fc.ASSUMED_GRID + 1)
    _, g = _check(rt, case)
    if case.n_new > _n_cu(rt) * fc.GRID_PER_CU:
        assert g["grid"] < case.n_new  # a workgroup takes a second row
    assert set(case.lengths.tolist()) <= {0, 1, 2}


# --------------------------------------------------------------------------
# d. repeated and shared fixed rows, clipped logits, a caller's init
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("special", fc.fold_cases()))
def test_special_rows(rt, name):
    case = fc.fold_cases()[name]
    got, _ = _check(rt, case)
    assert all(np.isfinite(a).all() for a in got)
    if case.with_init:
        assert np.abs(case.start()[0]).min() > 0


def test_bad_arguments(rt):
    from relevance_factorizationmachine_amd import _lib
    case = fc.fold_cases()["count1-k8"]
    k = case.k
    F, fL = case.fixed()
    g, l = case.feature_sums()
    dev = {n: rt.upload(a) for n, a in (("ptr", case.row_ptr), ("ids", case.ids if case.ids.size else np.zeros(1, np.int32)),
                                        ("ry", case.ry() if case.ids.size else np.zeros(1)), ("order", case.order),
                                        ("g", g), ("l", l), ("F", F), ("fL", fL), ("c", np.array([fc.C0])))}
    outs = {"w": fc.Guarded.blank(rt, 1), "V": fc.Guarded.blank(rt, k), "A": fc.Guarded.blank(rt, k),
            "L": fc.Guarded.blank(rt, 1)}

    def call(n_new=1, k=k, n_passes=1, n_fixed=case.n_fixed, **null):
        p = {n: (None if n in null else t.data_ptr()) for n, t in dev.items()}
        o = {n: (None if n in null else t.ptr) for n, t in outs.items()}
        return rt.lib.rfm_fm_fold_in(rt.ctx, p["ptr"], p["ids"], p["ry"], p["order"], n_new, p["g"], p["l"], p["F"], p["fL"],
                                     n_fixed, p["c"], k, case.lr, n_passes, o["w"], o["V"], o["A"], o["L"])
    for kw in (dict(k=0), dict(k=ms.MAX_FACTORS + 1), dict(n_new=-1), dict(n_passes=-1), dict(n_fixed=-1), dict(n_fixed=0),
               *(dict([(n, True)]) for n in list(dev) + list(outs))):
        assert call(**kw) == _lib.RFM_ERR_BAD_ARG, kw
        assert _lib.last_error(), kw
    # no rows is success, and nothing is written
    assert call(n_new=0) == _lib.RFM_OK
    rt.sync()
    for o in outs.values():
        o.host(written=0)


# --------------------------------------------------------------------------
# e. through Python: both sides, interleaved input, the flows
# --------------------------------------------------------------------------
def _flow(k, side="user"):
    """The small fit on the coat-shaped catalogue, loaded into a model: ``(model, sides, prob, lr, (w0, w, V))``."""
    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import recommend as rec
    prob = fc.flow_problem(k, side)
    w0, w, V = fc.flow_fit(prob)
    fit = {n: v for n, v in fc.FLOW_FIT.items() if n != "n_epochs"}
    model = pkg.FactorizationMachines(estimator="IPS", n_epochs=1, n_factors=k, seed=prob.seed, n_features=prob.n_features,
                                      **fit)
    for h, v in ((model.w0, w0), (model.w, w), (model.V, V)):
        h.set(v)
    return model, rec.Sides(prob.XU, prob.XI), prob, fc.flow_lr(prob, w, V), (w0, w, V)


def _grown_logits(prob, params, nu, om):
    """FM logits of every (user, item) pair of the grown catalogue on the grown model, by the CPU oracle:
    the new users' rows (user side) or every user over the grown items (item side)."""
    w0, w, V = params
    gw, gV = fc.grown_params(w, V, nu, om)
    XU, XI = fc.grown_sides(prob)
    u, i = fc.all_pairs(XU.shape[0], XI.shape[0], fc.FLOW_USERS if prob.side == "user" else 0)
    X = fc.pair_rows(XU, XI, u, i)
    return cpu_ref.fm_logit(X, w0, gw, gV).reshape(-1, XI.shape[0]), (w0, gw, gV), X


@pytest.mark.parametrize("side", ["user", "item"])
def test_python_both_sides_and_interleaved_input(rt, side):
    from relevance_factorizationmachine_amd import recommend as rec
    model, sides, prob, lr, params = _flow(12, side)
    fold = model.fold_in_users if side == "user" else model.fold_in_items
    folded = fold(sides, prob.new_rows, prob.data, prob.n_passes, lr=lr)
    assert folded.side == side and len(folded) == prob.n_new
    want = fc.flow_oracle(prob, *params, lr)
    d = fc.assert_within(folded.numpy(), want, fc.FMFOLD_TOL, f"flow {side}", lr)
    print(f"distance flow-{side} {d:.3e}")
    # the input's order between rows does not matter: grouped input gives the same bits
    col = 0 if side == "user" else 1
    by_row = np.argsort(prob.data["features"][:, col], kind="stable")
    assert (np.diff(prob.data["features"][:, col]) < 0).any()
    grouped = {n: v[by_row] for n, v in prob.data.items()}
    ops = rec.operands(model, sides)
    again = fold(sides, prob.new_rows, grouped, prob.n_passes, lr=lr, ops=ops)  # (and the operands reused)
    for a, b in zip(again.numpy() + (again.A.cpu().numpy(), again.L.cpu().numpy()),
                    folded.numpy() + (folded.A.cpu().numpy(), folded.L.cpu().numpy())):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    # lr: the model's unless given
    model.lr = lr
    for a, b in zip(fold(sides, prob.new_rows, prob.data, prob.n_passes).numpy(), folded.numpy()):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    model.lr = fc.FLOW_FIT["lr"]
    # a caller's init
    rng = np.random.default_rng(3)
    init = (rng.uniform(-0.2, 0.2, size=(prob.n_new, prob.k)), rng.normal(scale=0.1, size=prob.n_new))
    warm = fold(sides, prob.new_rows, prob.data, prob.n_passes, init=init, lr=lr)
    fc.assert_within(warm.numpy(), fc.flow_oracle(prob, *params, lr, start=init), fc.FMFOLD_TOL, f"flow {side} init", lr)
    idle = np.flatnonzero(np.asarray(fc.FLOW_LENGTHS) == 0)
    np.testing.assert_array_equal(_bits(warm.numpy()[0][idle]), _bits(init[0][idle]))
    # no passes: zeros stay zeros, the operands are the feature sums
    none = fold(sides, prob.new_rows, prob.data, 0, lr=lr)
    assert not none.numpy()[0].any() and not none.numpy()[1].any()
    g, l, _, _ = fc.flow_operands(prob, params[1], params[2], fc.LD)
    fc.assert_within((none.A.cpu().numpy()[:, :prob.k], none.L.cpu().numpy()), (g, l), fc.FMFOLD_TOL, "no passes", lr)
    # nothing of the model is written
    for h, v in zip((model.w0, model.w, model.V), params):
        np.testing.assert_array_equal(_bits(h()), _bits(v))
    with pytest.raises(IndexError):
        bad = np.array([[0, prob.n_fixed]]) if side == "user" else np.array([[prob.n_fixed, 0]])
        fold(sides, prob.new_rows, {"features": bad, "labels": np.ones(1), "pscores": np.ones(1)}, 1)
    with pytest.raises(ValueError):
        fold(sides, prob.new_rows, prob.data, 1, init=(np.zeros((1, prob.k)), np.zeros(1)))


@pytest.mark.parametrize("n_factors", [12, 13])  # the operands as they are, and zero-padded to 16
def test_flow_recommend_new_users(rt, n_factors):
    from relevance_factorizationmachine_amd import recommend as rec
    model, sides, prob, lr, params = _flow(n_factors)
    folded = model.fold_in_users(sides, prob.new_rows, prob.data, prob.n_passes, lr=lr)
    nu, om = folded.numpy()
    logits, grown, X = _grown_logits(prob, params, nu, om)  # on the folded values read back
    assert fc.smallest_gap(logits) > 1e-9
    n_items = fc.FLOW_ITEMS
    np.testing.assert_allclose(model.score_pairs(sides, new_users=folded),
                               cpu_ref.fm_predict(X, *grown).reshape(-1, n_items), rtol=1e-12)
    k = 7
    items, scores = model.recommend(sides, k, new_users=folded)
    np.testing.assert_array_equal(items, fc.ranking(logits, k))
    np.testing.assert_allclose(scores, cpu_ref.sigmoid(np.take_along_axis(logits, items.astype(np.int64), axis=1)), rtol=1e-12)
    deep, _, n_ranked = model.rank_catalogue(sides, n_items, new_users=folded)
    np.testing.assert_array_equal(deep, fc.ranking(logits, n_items))
    assert (n_ranked == n_items).all()
    # users and exclude index the folded rows
    sel = np.array([3, 0])
    excl = sp.csr_matrix((np.ones(prob.n_new), (np.arange(prob.n_new), items[:, 0])), shape=(prob.n_new, n_items))
    items_x, _ = model.recommend(sides, k - 1, users=sel, exclude=excl, new_users=folded)
    np.testing.assert_array_equal(items_x, items[sel, 1:])
    ranks, _, cand = model.rank_items(sides, np.arange(prob.n_new), items[:, 2], new_users=folded)
    assert (ranks == 2).all() and (cand == n_items).all()
    # the defaults still serve the catalogue's own users, and the model is not touched
    own, _ = model.recommend(sides, k)
    w0, w, V = params
    u, i = fc.all_pairs(fc.FLOW_USERS, n_items)
    np.testing.assert_array_equal(own, fc.ranking(cpu_ref.fm_logit(fc.pair_rows(prob.XU, prob.XI, u, i), w0, w, V)
                                                  .reshape(-1, n_items), k))
    assert model.n_features == prob.n_features and tuple(model.V.dev.shape) == (prob.n_features, n_factors)
    # into=: refreshed in place; buffers of another shape are refused
    import torch
    ops = rec.operands(model, sides, new_users=folded)
    assert ops.A.data_ptr() == folded.A.data_ptr() and tuple(ops.A.shape) == (prob.n_new, rec.pad4(n_factors))
    room = rec.Operands(rt, torch.zeros_like(folded.A), torch.zeros_like(folded.L), torch.zeros_like(ops.B),
                        torch.zeros_like(ops.LI), ops.c, n_factors)
    again = rec.operands(model, sides, into=room, new_users=folded)
    assert again.A.data_ptr() == room.A.data_ptr() and again.B.data_ptr() == room.B.data_ptr()
    np.testing.assert_array_equal(rec.topk(*again, k, None, None)[0], items)
    with pytest.raises(ValueError, match="into a buffer of"):
        rec.operands(model, sides, into=rec.operands(model, sides), new_users=folded)
    other = fc.flow_problem(n_factors, "item")  # (the same layout: its new item rows fit this catalogue)
    with pytest.raises(TypeError, match="Sides"):
        model.recommend(sides, 3, new_users=model.fold_in_items(sides, other.new_rows, other.data, 1, lr=lr))  # not users


def test_flow_append_columns_then_predict_recommend_fit(rt):
    from relevance_factorizationmachine_amd import recommend as rec
    model, sides, prob, lr, params = _flow(12)
    folded = model.fold_in_users(sides, prob.new_rows, prob.data, prob.n_passes, lr=lr)
    served_scores = model.score_pairs(sides, new_users=folded)
    served_items, _ = model.recommend(sides, 5, new_users=folded)
    ids = model.append_columns(folded)
    np.testing.assert_array_equal(ids, prob.n_features + np.arange(prob.n_new))
    assert model.n_features == prob.n_features + prob.n_new and model.V().shape == (model.n_features, 12)
    nu, om = folded.numpy()
    logits, grown, X = _grown_logits(prob, params, nu, om)
    for h, v in zip((model.w0, model.w, model.V), grown):
        np.testing.assert_array_equal(_bits(h()), _bits(v))
    # predict on rows that store the new columns
    np.testing.assert_allclose(model.predict(X), cpu_ref.fm_predict(X, *grown), rtol=1e-12)
    with pytest.raises(ValueError):
        model.predict(X[:, :-1])
    # the catalogue methods on Sides of the grown width agree with the new_users= route
    XU, XI = fc.grown_sides(prob)
    grown_sides = rec.Sides(XU, XI)
    new = fc.FLOW_USERS + np.arange(prob.n_new)
    np.testing.assert_allclose(model.score_pairs(grown_sides, users=new), served_scores, rtol=1e-12)
    np.testing.assert_array_equal(model.recommend(grown_sides, 5, users=new)[0], served_items)
    with pytest.raises(ValueError):
        model.recommend(sides, 5)  # (the catalogue of the old width)
    # one more fit iteration on the grown model, new users in the batch
    rng = np.random.default_rng(5)
    n = 60
    u, i = rng.integers(0, XU.shape[0], size=n), rng.integers(0, XI.shape[0], size=n)
    u[:prob.n_new] = new
    train = {"features": fc.pair_rows(XU, XI, u, i), "labels": (rng.random(n) < 0.5).astype(np.int64),
             "pscores": rng.uniform(0.1, 1.0, size=n) ** 0.5}
    val = {key: v[:20] for key, v in train.items()}
    model.fit(train, val)
    batch = cpu_ref.batch_ids(n, model.batch_size, 0)
    w0, gw, gV = (a.copy() for a in grown)
    cpu_ref.fm_step_closed(train["features"][batch], train["labels"][batch], train["pscores"][batch], w0, gw, gV, model.lr)
    assert np.abs(gV[prob.n_features:] - grown[2][prob.n_features:]).max() > 0  # the step moved the new columns
    for nm, v in zip(("w0", "w", "V"), (w0, gw, gV)):
        assert rel_err(getattr(model, nm)(), v) < TIGHT, nm
    with pytest.raises(TypeError):
        model.append_columns((nu, om))


def test_flow_append_items_then_recommend(rt):
    from relevance_factorizationmachine_amd import recommend as rec
    model, sides, prob, lr, params = _flow(12, "item")
    folded = model.fold_in_items(sides, prob.new_rows, prob.data, prob.n_passes, lr=lr)
    fc.assert_within(folded.numpy(), fc.flow_oracle(prob, *params, lr), fc.FMFOLD_TOL, "flow items", lr)
    ids = model.append_columns(folded)
    np.testing.assert_array_equal(ids, prob.n_features + np.arange(prob.n_new))
    nu, om = folded.numpy()
    logits, grown, X = _grown_logits(prob, params, nu, om)
    assert fc.smallest_gap(logits) > 1e-9
    XU, XI = fc.grown_sides(prob)
    n_items = fc.FLOW_ITEMS + prob.n_new
    items, scores = model.recommend(rec.Sides(XU, XI), n_items)  # every item of the grown catalogue, in order
    np.testing.assert_array_equal(items, fc.ranking(logits, n_items))
    assert all(set(range(fc.FLOW_ITEMS, n_items)) <= set(row.tolist()) for row in items)
    np.testing.assert_allclose(scores, cpu_ref.sigmoid(np.take_along_axis(logits, items.astype(np.int64), axis=1)), rtol=1e-12)
    np.testing.assert_allclose(model.predict(X), cpu_ref.fm_predict(X, *grown), rtol=1e-12)
