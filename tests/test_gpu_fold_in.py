"""MF fold-in on the device -- rfm_mf_fold_in through the raw C ABI against the long-double oracle of
fold_in_common.py, and fold_in_users / fold_in_items / append_* / new_users= through Python: at
every (lanes per row, vector width, chunks per lane) class of the kernel, with chains around both
depths of the read-ahead and a long chain beside short ones in one wavefront, under 0..3 passes, at
the row counts around a workgroup and past one pass of the capped grid, with repeated and shared
fixed rows, clipped logits and a caller's init.  Needs an MI355X: ``pytest -m gpu``.

Every case asserts the shape it means from rfm_mf_fold_geometry.  Every call is made twice from the
same start and must give the same bits (no atomics).  Rows are held to the oracle element by element
relative to their own row, biases relative to max(|c|, lr), at ``FOLD_TOL`` (derived from a CPU
measurement, see fold_in_common.py); a row without examples, the fixed side, the weights and the
sentinels around every array keep their bits.

On the code before fold-in every test here fails: the entry points do not exist."""
import numpy as np
import pytest
import scipy.sparse as sp

import fold_in_common as fc
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


def _check(rt, case, want=None):
    g = fc.geometry(case.n_new, case.k, rt)
    cls = ms.shape_class(case.k)
    assert (g["lpr"], g["vec"], g["nc"]) == cls and ms.CLASS_RANGE[cls][0] <= case.k <= ms.CLASS_RANGE[cls][1]
    assert g["rows"] == 256 // g["lpr"] and g["grid"] == min(-(-case.n_new // g["rows"]), _n_cu(rt) * fc.GRID_PER_CU)
    got = _twice(lambda: fc.run_fold(rt, case))
    d = fc.assert_within(got, fc.oracle(case) if want is None else want, fc.FOLD_TOL, case.name)
    print(f"distance {case.name} {d:.3e}")
    x0, c0 = case.start()
    idle = np.flatnonzero(case.lengths * case.n_passes == 0)
    np.testing.assert_array_equal(_bits(got[0][idle]), _bits(x0[idle]), err_msg="a row without examples changed")
    np.testing.assert_array_equal(_bits(got[1][idle]), _bits(c0[idle]), err_msg="a bias without examples changed")
    return got, g


# --------------------------------------------------------------------------
# a. every shape class at its lowest and highest factor count
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("shape-", fc.fold_cases()))
def test_every_shape_class(rt, name):
    case = fc.fold_cases()[name]
    _, g = _check(rt, case)
    d = g["depth"]
    assert {0, 1, d - 1, d, d + 1, 2 * d - 1, 2 * d, 2 * d + 1} <= set(case.lengths.tolist())
    per_wave = 64 // g["lpr"]
    if per_wave > 1:  # rows of different chain length share a wavefront
        first_wave = case.lengths[case.order[:per_wave]]
        assert len(set(first_wave.tolist())) > 1
    if g["lpr"] == 4:
        assert fc.LONG_CHAIN in case.lengths and case.n_new <= per_wave  # the long chain rides with the short ones


# --------------------------------------------------------------------------
# b. 0, 1, 2, 3 passes: the rings across the pass boundary
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("passes", fc.fold_cases()))
def test_passes(rt, name):
    case = fc.fold_cases()[name]
    got, _ = _check(rt, case)
    if case.n_passes == 0:
        for a, b in zip(got, case.start()):
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg="no passes changed a row")
    if case.n_passes >= 2:
        # passes are made one after the other, so p passes are p calls of one pass, bit for bit
        step = case.start()
        for _ in range(case.n_passes):
            step = fc.run_fold(rt, case, start=step, n_passes=1)
        for a, b in zip(got, step):
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg="one call of p passes and p calls of one differ")


# --------------------------------------------------------------------------
# c. row counts around a workgroup, and past one pass of the capped grid
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("count", fc.fold_cases()))
def test_row_counts(rt, name):
    case = fc.fold_cases()[name]
    _, g = _check(rt, case)
    assert case.n_new in (1, g["rows"] - 1, g["rows"], g["rows"] + 1)
    assert g["grid"] == (2 if case.n_new == g["rows"] + 1 else 1)


def test_grid_stride(rt):
    case = fc.grid_case(_n_cu(rt))
    _, g = _check(rt, case, fc.fold_all(case))
    assert g["grid"] == _n_cu(rt) * fc.GRID_PER_CU and case.n_new == g["grid"] * g["rows"] + 37


# --------------------------------------------------------------------------
# d. repeated and shared fixed rows, clipped logits, a caller's init
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("special", fc.fold_cases()))
def test_special_chains(rt, name):
    case = fc.fold_cases()[name]
    got, _ = _check(rt, case)
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    if case.with_init:
        assert np.abs(case.start()[0]).min() > 0


def test_bad_arguments(rt):
    from relevance_factorizationmachine_amd import _lib
    case = fc.fold_cases()["count1-k16"]
    F, fb = case.fixed()
    dev = {n: rt.upload(a) for n, a in (("ptr", case.row_ptr), ("ids", case.ids), ("ry", case.ry()), ("order", case.order),
                                        ("F", F), ("fb", fb))}
    rows, bias = fc.Guarded.blank(rt, case.k), fc.Guarded.blank(rt, 1)

    def call(n_new=1, k=case.k, n_passes=1, n_fixed=case.n_fixed, **null):
        p = {n: (None if n in null else t.data_ptr()) for n, t in dev.items()}
        return rt.lib.rfm_mf_fold_in(rt.ctx, p["ptr"], p["ids"], p["ry"], p["order"], n_new, p["F"], p["fb"], n_fixed,
                                     ms.B0, k, ms.LR, ms.REG, n_passes, None if "rows" in null else rows.ptr,
                                     None if "bias" in null else bias.ptr)
    for kw in (dict(k=0), dict(k=ms.MAX_FACTORS + 1), dict(n_new=-1), dict(n_passes=-1), dict(n_fixed=-1), dict(n_fixed=0),
               *(dict([(n, True)]) for n in ("ptr", "ids", "ry", "order", "F", "fb", "rows", "bias"))):
        assert call(**kw) == _lib.RFM_ERR_BAD_ARG, kw
        assert _lib.last_error(), kw
    # nothing to do is success, and nothing is written
    assert call(n_new=0) == _lib.RFM_OK and call(n_passes=0) == _lib.RFM_OK
    rt.sync()
    rows.host(written=0), bias.host(written=0)


# --------------------------------------------------------------------------
# e. through Python: both sides, interleaved input, the three flows
# --------------------------------------------------------------------------
N_OLD, N_ITEMS, FLOW_K = 9, 20, 12


def _flow_case(name="flow", n_fixed=N_ITEMS, with_init=False, k=FLOW_K):
    lengths = [6, 0, 3, 11, 2]
    return fc.FoldCase(name, k, fc._chains(name, lengths, n_fixed), 2, with_init=with_init, n_fixed=n_fixed)


def _model(n_users, n_items, P, Q, bu, bi, n_epochs=1, batch_size=40):
    import relevance_factorizationmachine_amd as pkg
    m = pkg.LogisticMatrixFactorization(estimator="IPS", n_epochs=n_epochs, n_factors=P.shape[1], lr=ms.LR,
                                        batch_size=batch_size, seed=3, n_users=n_users, n_items=n_items, reg=ms.REG)
    for h, v in ((m.P, P), (m.Q, Q), (m.b_u, bu), (m.b_i, bi)):
        h.set(v)
    m.b = ms.B0
    return m


def _user_side_model(case):
    F, fb = case.fixed()
    P, _, bu, _ = cpu_ref.mf_init(11, N_OLD, 1, case.k)
    return _model(N_OLD, case.n_fixed, P, F, bu, fb), (P, F, bu, fb)


def _logits(P, Q, bu, bi):
    return np.asarray(P, dtype=np.float64) @ np.asarray(Q, dtype=np.float64).T + np.asarray(bu, dtype=np.float64)[:, None] \
        + np.asarray(bi, dtype=np.float64)[None, :] + ms.B0


def _ranking(logits, k):
    """recommend()'s order: logit descending, ties the higher item index first."""
    return np.argsort(logits, axis=1, kind="stable")[:, ::-1][:, :k]


def test_python_both_sides_and_interleaved_input(rt):
    for with_init in (False, True):
        case = _flow_case(with_init=with_init)
        abi = fc.run_fold(rt, case)
        fc.assert_within(abi, fc.oracle(case), fc.FOLD_TOL, case.name)
        init = case.start() if with_init else None
        model, params = _user_side_model(case)
        for interleaved in (False, True):
            folded = model.fold_in_users(case.data("user", interleaved), case.n_new, case.n_passes, init=init)
            assert folded.side == "user" and len(folded) == case.n_new
            for a, b in zip(folded.numpy(), abi):
                np.testing.assert_array_equal(_bits(a), _bits(b), err_msg="Python and the raw call differ")
        # nothing of the model is written
        for h, v in zip((model.P, model.Q, model.b_u, model.b_i), params):
            np.testing.assert_array_equal(_bits(h()), _bits(v))
        # the item side is the same rule on the model with P <-> Q, b_u <-> b_i and the columns exchanged
        P, F, bu, fb = params
        mirror = _model(case.n_fixed, 3, F, np.zeros((3, case.k)), fb, np.zeros(3))
        folded = mirror.fold_in_items(case.data("item", True), case.n_new, case.n_passes, init=init)
        assert folded.side == "item"
        for a, b in zip(folded.numpy(), abi):
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg="the item side and the mirrored user side differ")
    with pytest.raises(IndexError):
        model.fold_in_users({"features": np.array([[0, N_ITEMS]]), "labels": np.ones(1), "pscores": np.ones(1)}, 1, 1)
    with pytest.raises(ValueError):
        model.fold_in_users(case.data(), case.n_new, 1, init=(np.zeros((1, case.k)), np.zeros(1)))
    empty = model.fold_in_users(case.data(), case.n_new, 0)
    assert not empty.numpy()[0].any() and not empty.numpy()[1].any()


@pytest.mark.parametrize("n_factors", [FLOW_K, FLOW_K + 1])  # the operands as they are, and zero-padded to 16
def test_flow_recommend_new_users(rt, n_factors):
    case = _flow_case(k=n_factors)
    model, (P, Q, bu, bi) = _user_side_model(case)
    folded = model.fold_in_users(case.data("user", True), case.n_new, case.n_passes)
    want_rows, want_bias = fc.oracle(case)
    logits = _logits(want_rows, Q, want_bias, bi)  # score_pairs' definition on the oracle's rows
    k = 7
    items, scores = model.recommend(k, new_users=folded)
    np.testing.assert_array_equal(items, _ranking(logits, k))
    np.testing.assert_allclose(scores, cpu_ref.sigmoid(np.take_along_axis(logits, items.astype(np.int64), axis=1)), rtol=1e-12)
    np.testing.assert_allclose(model.score_pairs(new_users=folded), cpu_ref.sigmoid(logits), rtol=1e-12)
    # users and exclude index the folded rows
    sel = np.array([3, 0])
    excl = sp.csr_matrix((np.ones(case.n_new), (np.arange(case.n_new), items[:, 0])), shape=(case.n_new, N_ITEMS))
    items_x, _ = model.recommend(k - 1, users=sel, exclude=excl, new_users=folded)
    np.testing.assert_array_equal(items_x, items[sel, 1:])
    ranks, _, cand = model.rank_items(np.arange(case.n_new), items[:, 2], new_users=folded)
    assert (ranks == 2).all() and (cand == N_ITEMS).all()
    deep, _, n_ranked = model.rank_catalogue(N_ITEMS, new_users=folded)
    np.testing.assert_array_equal(deep, _ranking(logits, N_ITEMS))
    assert (n_ranked == N_ITEMS).all()
    # the defaults still serve the model's own users
    own, _ = model.recommend(k)
    np.testing.assert_array_equal(own, _ranking(_logits(P, Q, bu, bi), k))
    assert model.n_users == N_OLD and tuple(model.P.dev.shape) == (N_OLD, case.k)
    # into=: the operands of the same folded rows are refreshed in place; those of the model's own
    # users have other shapes when the rows are padded, and are refused
    from relevance_factorizationmachine_amd import recommend as rec
    ops = rec.operands(model, new_users=folded)
    again = rec.operands(model, into=ops, new_users=folded)
    assert again.A.data_ptr() == ops.A.data_ptr() and tuple(again.A.shape) == (case.n_new, rec.pad4(case.k))
    np.testing.assert_array_equal(rec.topk(*again, k, None, None)[0], items)
    if case.k % 4:
        with pytest.raises(ValueError, match="into a buffer of"):
            rec.operands(model, into=rec.operands(model), new_users=folded)


def test_flow_append_users_then_predict_recommend_fit(rt):
    case = _flow_case()
    model, (P, Q, bu, bi) = _user_side_model(case)
    folded = model.fold_in_users(case.data(), case.n_new, case.n_passes)
    served, _ = model.recommend(5, new_users=folded)
    ids = model.append_users(folded)
    np.testing.assert_array_equal(ids, N_OLD + np.arange(case.n_new))
    assert model.n_users == N_OLD + case.n_new and model.P().shape == (model.n_users, case.k)
    rows, bias = folded.numpy()
    grown = [np.concatenate([P, rows]), Q.copy(), np.concatenate([bu, bias]), bi.copy()]
    for h, v in zip((model.P, model.Q, model.b_u, model.b_i), grown):
        np.testing.assert_array_equal(_bits(h()), _bits(v))
    pairs = np.stack([np.repeat(ids, 3), np.tile([0, 7, 19], len(ids))], axis=1)
    np.testing.assert_allclose(model.predict(pairs), cpu_ref.mf_predict(pairs, *grown, ms.B0), rtol=1e-12)
    with pytest.raises(IndexError):
        model.predict(np.array([[model.n_users, 0]]))
    again, _ = model.recommend(5, users=ids)
    np.testing.assert_array_equal(again, served)
    # one more fit iteration on the grown model, new users in the batch
    rng = np.random.default_rng(5)
    n = 120
    train = {"features": np.stack([rng.integers(0, model.n_users, size=n), rng.integers(0, N_ITEMS, size=n)], axis=1),
             "labels": (rng.random(n) < 0.5).astype(np.int64), "pscores": rng.uniform(0.1, 1.0, size=n) ** 0.5}
    train["features"][:case.n_new, 0] = ids
    val = {k: v[:30] for k, v in train.items()}
    model.fit(train, val)
    b = float(np.mean(train["labels"]))
    batch = cpu_ref.batch_ids(n, model.batch_size, 0)
    cpu_ref.mf_sgd_batch(train["features"][batch], train["labels"][batch], train["pscores"][batch], *grown, b, ms.LR,
                         ms.REG)
    for nm, v in zip(("P", "Q", "b_u", "b_i"), grown):
        assert rel_err(getattr(model, nm)(), v) < TIGHT, nm
    with pytest.raises(TypeError):
        model.append_items(folded)


def test_flow_append_items_then_recommend(rt):
    case = _flow_case("flow-items", n_fixed=N_OLD)
    F, fb = case.fixed()                               # the users are the fixed side here
    _, Q, _, bi = cpu_ref.mf_init(13, 1, N_ITEMS, case.k)
    model = _model(N_OLD, N_ITEMS, F, Q, fb, bi)
    folded = model.fold_in_items(case.data("item", True), case.n_new, case.n_passes)
    fc.assert_within(folded.numpy(), fc.oracle(case), fc.FOLD_TOL, case.name)
    ids = model.append_items(folded)
    np.testing.assert_array_equal(ids, N_ITEMS + np.arange(case.n_new))
    assert model.n_items == N_ITEMS + case.n_new
    rows, bias = folded.numpy()
    logits = _logits(F, np.concatenate([Q, rows]), fb, np.concatenate([bi, bias]))
    items, scores = model.recommend(model.n_items)     # every item of the grown catalogue, in order
    np.testing.assert_array_equal(items, _ranking(logits, model.n_items))
    assert all(set(ids.tolist()) <= set(row.tolist()) for row in items)
    np.testing.assert_allclose(scores, cpu_ref.sigmoid(np.take_along_axis(logits, items.astype(np.int64), axis=1)), rtol=1e-12)
    with pytest.raises(TypeError):
        model.recommend(3, new_users=folded)           # folded items are not users
