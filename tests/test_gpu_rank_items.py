"""Ranks against the whole catalogue on the device: ``rank_items`` of
``FactorizationMachines`` / ``LogisticMatrixFactorization``, ``evaluate.CatalogueEvaluator`` and
``rfm_pair_ranks`` through the C ABI.  Needs an MI355X: ``pytest -m gpu``.  The ranks are integers
and are compared EXACTLY, every pair of every fixture model; the fixture is that of
``test_gpu_recommend.py`` (``tests/golden/recommend*.npz``), the tolerances on the scores are that
file's, unchanged."""
import numpy as np
import pytest
from scipy import sparse as sp

import rank_items_common as rk
import recommend_common as rc
import test_gpu_recommend as tgr
from conftest import load_golden
from relevance_factorizationmachine_amd import synth

pytestmark = pytest.mark.gpu

NU, NI = rc.N_USERS, rc.N_ITEMS


@pytest.fixture(scope="module")
def rfm():
    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import features, recommend, runtime
    return pkg, features, recommend, runtime.Runtime.get()


@pytest.fixture(scope="module")
def gold():
    return load_golden("recommend"), {layout: load_golden(f"recommend_fm_{layout}") for layout in rc.LAYOUTS}


def _device_model(rfm, gold, model):
    """``(rank_items(users, items, exclude=None), recommend(k, users=None, exclude=None), R)`` of a fixture model."""
    kind, layout, k, alpha = model
    if kind == "mf":
        m = tgr._mf_model(rfm[0], gold[0], k)
        return m.rank_items, m.recommend, gold[0][f"mf_k{k}_R"]
    m, sides, R, _ = tgr._fixture_model(rfm, gold, layout, k, alpha)
    return (lambda *a, **kw: m.rank_items(sides, *a, **kw)), (lambda *a, **kw: m.recommend(sides, *a, **kw)), R


# --------------------------------------------------------------------------- 3
@pytest.mark.parametrize("model", rk.MODELS, ids=rk.model_id)
def test_every_pair_of_every_fixture_model_exactly(rfm, gold, model):
    rank_items, _, R = _device_model(rfm, gold, model)
    Z = rk.model_logits(gold[0], gold[1], model)
    gap = rk.min_relative_gap(Z)
    print(rk.model_id(model), "smallest relative gap between neighbouring logits of a user:", gap)
    assert gap > 1e-9  # the exact comparison below is not a coin toss
    uu, ii = rc.all_pairs(NU, NI)
    ranks, scores, cand = rank_items(uu, ii)
    assert ranks.shape == scores.shape == cand.shape == (NU * NI,)
    assert ranks.dtype == np.int32 and scores.dtype == np.float64 and cand.dtype == np.int32
    want = np.stack([rk.ranks_by_argsort(Z[u]) for u in range(NU)])
    np.testing.assert_array_equal(ranks.reshape(NU, NI), want)  # every pair, none left out
    np.testing.assert_array_equal(cand, NI)
    tgr._close(scores.reshape(NU, NI), R, rk.model_id(model))
    # any order of the pairs, repeats: the same answers at the same places
    rng = np.random.default_rng(model[2])
    pick = rng.integers(0, NU * NI, size=500)
    r2, s2, c2 = rank_items(uu[pick], ii[pick])
    np.testing.assert_array_equal(r2, ranks[pick])
    assert s2.tobytes() == scores[pick].tobytes()
    np.testing.assert_array_equal(c2, NI)


def test_saturated_probabilities_still_rank_exactly(rfm, gold):
    """alpha = 2.0: a share of the probabilities is exactly 0.0 / 1.0, so ranks taken from
    ``score_pairs()`` on the host tie where the logits do not."""
    model = ("fm", "kuairec", 16, 2.0)
    rank_items, _, R = _device_model(rfm, gold, model)
    assert float(np.mean((R == 0.0) | (R == 1.0))) > 0.02
    Z = rk.model_logits(gold[0], gold[1], model)
    uu, ii = rc.all_pairs(NU, NI)
    ranks = rank_items(uu, ii)[0].reshape(NU, NI)
    from_probabilities = np.stack([rk.ranks_by_argsort(R[u]) for u in range(NU)])
    np.testing.assert_array_equal(ranks, np.stack([rk.ranks_by_argsort(Z[u]) for u in range(NU)]))
    assert (from_probabilities != ranks).any()


# --------------------------------------------------------------------------- 4
def _assert_ranks_of_recommendations(rank_items, recommend, K, users, exclude, what):
    items, scores = recommend(K, users=users, exclude=exclude)
    ok = items >= 0
    rows = np.repeat(np.arange(NU) if users is None else np.asarray(users), K).reshape(items.shape)
    ranks, rscores, cand = rank_items(rows[ok], items[ok], exclude=exclude)
    np.testing.assert_array_equal(ranks, np.tile(np.arange(K), (items.shape[0], 1))[ok], err_msg=what)
    assert rscores.tobytes() == scores[ok].tobytes(), what  # the same logit bits through the same sigmoid
    return items, cand.astype(np.int64), rows[ok]


@pytest.mark.parametrize("K", [1, 9, 64])
@pytest.mark.parametrize("model", rk.MODELS, ids=rk.model_id)
def test_rank_of_the_r_th_recommendation_is_r(rfm, gold, model, K):
    rank_items, recommend, _ = _device_model(rfm, gold, model)
    _, cand, _ = _assert_ranks_of_recommendations(rank_items, recommend, K, None, None, "no exclusion")
    assert (cand == NI).all()
    _assert_ranks_of_recommendations(rank_items, recommend, K, tgr.SUBSET, None, "subset")
    train = rk.heldout(gold[0])[0]
    E = sp.csr_matrix(train.astype(np.float64))
    for exclude in (E, (E.indptr, E.indices)):
        items, cand, rows = _assert_ranks_of_recommendations(rank_items, recommend, K, None, exclude, "train pairs excluded")
        assert not train[rows, items[items >= 0]].any()
        np.testing.assert_array_equal(cand, (NI - train.sum(axis=1))[rows])
    # lists like those of test_gpu_recommend.test_exclusions: a user who keeps 3 items, one who keeps none
    M = np.random.default_rng(11).random((NU, NI)) < 0.3
    M[4] = True
    M[4, [3, 77, 150]] = False
    M[9] = True
    M[12] = False
    items, cand, rows = _assert_ranks_of_recommendations(rank_items, recommend, K, None, sp.csr_matrix(M.astype(np.float64)), "random lists")
    assert (items[9] == -1).all() and (items[4] >= 0).sum() == min(K, 3)
    np.testing.assert_array_equal(cand, (NI - M.sum(axis=1))[rows])


@pytest.mark.parametrize("k,alpha", [(32, 2.0), (400, 0.25)])
def test_consistency_with_recommend_at_catalogue_size(rfm, k, alpha):
    pkg, features, recommend, rt = rfm
    sh = synth.SHAPES["kuairec_small"]
    nu, ni = sh.n_users, sh.n_items
    user, item, ctx = tgr._kuairec_tables(np.random.default_rng(k), nu, ni)
    sides = features.sides_kuairec(rt, nu, ni, ctx, user, item)
    model = pkg.FactorizationMachines(estimator="IPS", n_epochs=1, n_factors=k, n_features=sides.n_features,
                                      lr=1e-4, batch_size=1, seed=7, alpha=alpha)
    K = 64
    items, scores = model.recommend(sides, k=K)
    assert (items >= 0).all()
    uu = np.repeat(np.arange(nu), K)
    ranks, rscores, cand = model.rank_items(sides, uu, items.ravel())
    np.testing.assert_array_equal(ranks.reshape(nu, K), np.tile(np.arange(K), (nu, 1)))
    assert rscores.tobytes() == scores.tobytes()
    np.testing.assert_array_equal(cand, ni)
    # the user list three times over: 67 user tiles instead of 23, so another cut of the items into
    # splits (the number of splits goes by the number of user tiles) -- the counts are integers
    order = np.argsort(items, axis=1)
    sel = np.tile(np.arange(nu), 3).astype(np.int32)
    indptr = np.arange(3 * nu + 1, dtype=np.int64) * K
    tgt = np.tile(np.take_along_axis(items, order, axis=1), (3, 1)).astype(np.int32).ravel()
    r3, s3, c3 = recommend._rank_grouped(*recommend.operands(model, sides), sel, indptr, tgt, None)
    np.testing.assert_array_equal(r3.reshape(3 * nu, K), np.tile(order, (3, 1)))
    np.testing.assert_array_equal(c3, ni)
    assert s3.reshape(3 * nu, K).tobytes() == np.tile(np.take_along_axis(scores, order, axis=1), (3, 1)).tobytes()
    # deeper than recommend() reaches: ranks of a user's items 0 .. 299 are 300 different positions
    # below the catalogue size, and the items that recommend() returned are the ones ranked < 64
    deep_u, deep_i = np.repeat(np.arange(5), 300), np.tile(np.arange(300), 5)
    deep = model.rank_items(sides, deep_u, deep_i)[0].reshape(5, 300)
    for u in range(5):
        assert len(set(deep[u].tolist())) == 300 and deep[u].min() >= 0 and deep[u].max() < ni
        assert set(np.flatnonzero(deep[u] < K).tolist()) == set(items[u][items[u] < 300].tolist())


# --------------------------------------------------------------------------- 5
def _abi_ranks(rfm, A, LU, B, LI, c, tgt_indptr, tgt_items, user_ids=None, excl=None, n_sel=None, raw=None):
    _, _, recommend, rt = rfm
    import torch
    from relevance_factorizationmachine_amd import _lib
    kf = A.shape[1]
    dA, dB = recommend.padded(rt, rt.upload(A), kf), recommend.padded(rt, rt.upload(B), kf)
    dLU, dLI, dc = rt.upload(LU), rt.upload(LI), rt.upload(np.array([c], dtype=np.float64))
    ids = None if user_ids is None else rt.upload(np.asarray(user_ids, dtype=np.int32))
    if n_sel is None:
        n_sel = A.shape[0] if user_ids is None else len(user_ids)
    tgt_indptr, tgt_items = np.asarray(tgt_indptr, dtype=np.int64), np.asarray(tgt_items, dtype=np.int32)
    n_tgt = int(tgt_items.shape[0])
    d_indptr = rt.upload(tgt_indptr)
    d_items = rt.upload(tgt_items) if n_tgt else None
    ws = rt.empty((recommend.ranks_workspace_bytes(n_sel, B.shape[0], n_tgt),), torch.uint8)
    ranks, scores = rt.empty((max(n_tgt, 1),), torch.int32), rt.empty((max(n_tgt, 1),), torch.float64)
    cand = rt.empty((max(n_sel, 1),), torch.int32)
    ex = (None, None) if excl is None else (rt.upload(excl[0].astype(np.int64)), rt.upload(excl[1].astype(np.int32)))
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    args = dict(ctx=rt.ctx, A=dA.data_ptr(), LU=dLU.data_ptr(), n_users=A.shape[0], ids=ptr(ids), n_sel=n_sel,
                B=dB.data_ptr(), LI=dLI.data_ptr(), n_items=B.shape[0], kf=kf, c=dc.data_ptr(), ei=ptr(ex[0]),
                ex=ptr(ex[1]), ti=d_indptr.data_ptr(), tx=ptr(d_items), ws=ws.data_ptr() if n_tgt else None,
                ranks=ranks.data_ptr() if n_tgt else None, scores=scores.data_ptr() if n_tgt else None,
                cand=cand.data_ptr())
    args.update(raw or {})
    _lib.check(rt.lib.rfm_pair_ranks(*args.values()))
    rt.sync()
    return ranks.cpu().numpy()[:n_tgt], scores.cpu().numpy()[:n_tgt], cand.cpu().numpy()[:n_sel]


def _order_rule_operands(n_users, n_items, kf):
    """The operands of test_gpu_recommend.test_order_rule_and_determinism_through_the_abi."""
    rng = np.random.default_rng(n_users * 1000 + n_items)
    A = rng.integers(-2, 3, size=(n_users, kf)).astype(np.float64)
    B = rng.integers(-2, 3, size=(n_items, kf)).astype(np.float64)
    LU = rng.integers(-1, 2, size=n_users).astype(np.float64)
    LI = rng.integers(-1, 2, size=n_items).astype(np.float64)
    A[1] = 0.0
    LI[:] = np.where(rng.random(n_items) < 0.5, 0.0, LI)
    B[n_items // 2] = np.nan
    c = 3.0
    logit = c + LU[:, None] + LI[None, :] + A @ B.T
    logit[:, n_items // 2] = np.nan
    return rng, A, LU, B, LI, c, logit


def _expected(logit, sel, tgt_indptr, tgt_items, mask=None):
    ranks, scores, cand = [], [], []
    for s, u in enumerate(sel):
        r, n = rk.ranks_by_definition(logit[u], None if mask is None else mask[u])
        mine = tgt_items[tgt_indptr[s]:tgt_indptr[s + 1]]
        ranks.append(r[mine])
        scores.append(rc.sigmoid(logit[u, mine]))
        cand.append(n)
    return np.concatenate(ranks), np.concatenate(scores), np.array(cand)


def _check(got, want, what):
    ranks, scores, cand = got
    np.testing.assert_array_equal(ranks, want[0], err_msg=what)
    np.testing.assert_array_equal(cand, want[2], err_msg=what)
    np.testing.assert_array_equal(np.isnan(scores), want[0] < 0, err_msg=what)
    ok = want[0] >= 0
    if ok.any():
        tgr._close(scores[ok], want[1][ok], what)


@pytest.mark.parametrize("n_users,n_items,kf", [(70, 150, 6), (3, 5, 4), (130, 64, 5), (64, 321, 9)])
def test_order_rule_and_determinism_through_the_abi(rfm, n_users, n_items, kf):
    rng, A, LU, B, LI, c, logit = _order_rule_operands(n_users, n_items, kf)
    if n_items >= 64:
        assert (np.diff(np.sort(logit[0][~np.isnan(logit[0])])) == 0).any()  # ties exist
    users = np.arange(n_users)
    indptr, tgt = np.arange(n_users + 1) * n_items, np.tile(np.arange(n_items), n_users)  # all pairs
    got = _abi_ranks(rfm, A, LU, B, LI, c, indptr, tgt)
    want = _expected(logit, users, indptr, tgt)
    _check(got, want, "all pairs")
    assert (got[0].reshape(n_users, n_items)[:, n_items // 2] == -1).all() and (got[2] == n_items - 1).all()
    # a total order: every user's ranks are a permutation (user 1 has A = 0: ties all over)
    np.testing.assert_array_equal(np.sort(got[0].reshape(n_users, n_items), axis=1),
                                  np.tile(np.arange(-1, n_items - 1), (n_users, 1)))
    again = _abi_ranks(rfm, A, LU, B, LI, c, indptr, tgt)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))  # identical bits, NaN scores included
    # random exclusion lists: fewer candidates, smaller ranks; an excluded target is still ranked
    M = rng.random((n_users, n_items)) < 0.3
    M[0] = False
    M[n_users - 1] = True
    E = sp.csr_matrix(M.astype(np.float64))
    got_e = _abi_ranks(rfm, A, LU, B, LI, c, indptr, tgt, excl=(E.indptr, E.indices))
    want_e = _expected(logit, users, indptr, tgt, M)
    _check(got_e, want_e, "all pairs, exclusion lists")
    np.testing.assert_array_equal(got_e[2], (~M & ~np.isnan(logit)).sum(axis=1))
    assert (got_e[0] <= got[0]).all() and got_e[2][n_users - 1] == 0
    assert (got_e[0].reshape(n_users, n_items)[n_users - 1][~np.isnan(logit[n_users - 1])] == 0).all()
    # a permuted, repeating user list; per selected user a few targets, some twice, some none
    sel = rng.integers(0, n_users, size=n_users + 7)
    counts = rng.integers(0, 2 * n_items, size=sel.shape[0])
    counts[0] = 0
    indptr2 = np.concatenate(([0], np.cumsum(counts)))
    tgt2 = np.concatenate([np.sort(rng.integers(0, n_items, size=n)) for n in counts])
    got2 = _abi_ranks(rfm, A, LU, B, LI, c, indptr2, tgt2, user_ids=sel, excl=(E.indptr, E.indices))
    _check(got2, _expected(logit, sel, indptr2, tgt2, M), "repeated targets, permuted users")
    again2 = _abi_ranks(rfm, A, LU, B, LI, c, indptr2, tgt2, user_ids=sel, excl=(E.indptr, E.indices))
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got2, again2))


def test_more_targets_than_a_workgroup_sums_in_lds(rfm):
    """64 users x 321 items x 4 repeats = 82 176 targets in one user tile: beyond the first 4 096
    the counts are added to memory per tile; the result is the same integers."""
    _, A, LU, B, LI, c, logit = _order_rule_operands(64, 321, 9)
    indptr, tgt = np.arange(65) * 4 * 321, np.tile(np.repeat(np.arange(321), 4), 64)
    _check(_abi_ranks(rfm, A, LU, B, LI, c, indptr, tgt), _expected(logit, np.arange(64), indptr, tgt), "4 x all pairs")


# --------------------------------------------------------------------------- 6
@pytest.mark.parametrize("model", [("fm", "kuairec", 33, 0.25), ("fm", "coat", 16, 2.0), ("mf", None, 24, None)],
                         ids=rk.model_id)
def test_heldout_evaluation_end_to_end(rfm, gold, model):
    from relevance_factorizationmachine_amd.evaluate import CatalogueEvaluator

    g = gold[0]
    train, positives, dropped = rk.heldout(g)
    assert train.sum() == 1853 and train.sum(axis=1).max() == 45
    assert positives[0].shape[0] + dropped[0].shape[0] == 103 and dropped[0].shape[0] == 13
    assert positives[0].shape[0] == 90 and np.unique(positives[0]).shape[0] == 45
    E = sp.csr_matrix(train.astype(np.float64))
    if model[0] == "mf":
        m, sides = tgr._mf_model(rfm[0], g, model[2]), None
    else:
        m, sides, _, _ = tgr._fixture_model(rfm, gold, *model[1:])
    ev = CatalogueEvaluator(positives, NI, rk.K_LIST, rk.METRICS, exclude=E)
    got = ev.evaluate(m, sides)
    assert ev.unranked == 0
    Z = rk.model_logits(g, gold[1], model)
    rk.assert_metrics_equal(got, rk.oracle_metrics(Z, positives, train), rk.model_id(model))
    # without the exclusion lists the train pairs compete: another, equally exact, answer
    got_all = CatalogueEvaluator(positives, NI, rk.K_LIST, rk.METRICS).evaluate(m, sides)
    rk.assert_metrics_equal(got_all, rk.oracle_metrics(Z, positives, np.zeros_like(train)), rk.model_id(model) + " no exclusion")
    # a positive that the exclusion lists name has no rank
    everything = (np.concatenate([positives[0], dropped[0]]), np.concatenate([positives[1], dropped[1]]))
    with pytest.raises(ValueError, match="exclusion list"):
        CatalogueEvaluator(everything, NI, rk.K_LIST, rk.METRICS, exclude=E).evaluate(m, sides)


# --------------------------------------------------------------------------- 7
def test_abi_rejects_bad_arguments(rfm):
    A, B = np.ones((3, 4)), np.ones((5, 4))
    ok = dict(tgt_indptr=[0, 1, 2], tgt_items=[0, 4], user_ids=[0, 1])
    _abi_ranks(rfm, A, np.zeros(3), B, np.zeros(5), 0.0, **ok)
    for raw, match in (({"ti": None}, "null"), ({"cand": None}, "null"), ({"tx": None}, "null"),
                       ({"ws": None}, "null"), ({"ranks": None}, "null"), ({"scores": None}, "null"),
                       ({"kf": 0}, "n_factors"), ({"A": None}, "null"), ({"ids": None}, "every user is selected"),
                       ({"ei": rfm[3].upload(np.zeros(4, np.int64)).data_ptr()}, "exclusion lists without items"),
                       ({"n_sel": -1}, "n_sel_users")):
        with pytest.raises(ValueError, match=match):
            _abi_ranks(rfm, A, np.zeros(3), B, np.zeros(5), 0.0, raw=raw, **ok)


def test_no_targets_still_counts_the_candidates(rfm):
    _, A, LU, B, LI, c, logit = _order_rule_operands(70, 150, 6)
    ranks, scores, cand = _abi_ranks(rfm, A, LU, B, LI, c, np.zeros(71, np.int64), np.zeros(0, np.int32))
    assert ranks.shape == scores.shape == (0,)
    np.testing.assert_array_equal(cand, 149)
    sel = [3, 3, 69]
    ranks, scores, cand = _abi_ranks(rfm, A, LU, B, LI, c, np.zeros(4, np.int64), np.zeros(0, np.int32), user_ids=sel)
    np.testing.assert_array_equal(cand, [149, 149, 149])
    # no selected user: nothing to do
    _abi_ranks(rfm, A, LU, B, LI, c, np.zeros(1, np.int64), np.zeros(0, np.int32), user_ids=[0], n_sel=0)


def test_ids_outside_their_tables(rfm, monkeypatch):
    """Never read out of bounds: a user id outside the table ranks nothing (rank -1, score NaN, no
    candidates), an item id outside the catalogue has rank -1 / score NaN; with RFM_CHECK_IDS=1
    both, and a target list that is not ascending, are errors."""
    rng = np.random.default_rng(5)
    A, B = rng.integers(-2, 3, size=(3, 4)).astype(np.float64), rng.integers(-2, 3, size=(6, 4)).astype(np.float64)
    LU, LI = np.zeros(3), np.arange(6.0)
    logit = 1.0 + LI[None, :] + A @ B.T
    monkeypatch.delenv("RFM_CHECK_IDS", raising=False)
    sel = [1, 3, -1, 0]
    indptr, tgt = [0, 2, 4, 5, 7], [0, 5, 1, 2, 3, 2, 4]
    ranks, scores, cand = _abi_ranks(rfm, A, LU, B, LI, 1.0, indptr, tgt, user_ids=sel)
    np.testing.assert_array_equal(cand, [6, 0, 0, 6])
    np.testing.assert_array_equal(ranks, [*rk.ranks_by_definition(logit[1])[0][[0, 5]], -1, -1, -1,
                                          *rk.ranks_by_definition(logit[0])[0][[2, 4]]])
    np.testing.assert_array_equal(np.isnan(scores), ranks < 0)
    # item ids below, just above (inside the last tile's padding) and far above the catalogue
    indptr, tgt = [0, 5, 5, 7], [-3, 2, 6, 63, 5000, 0, 64]
    ranks, scores, cand = _abi_ranks(rfm, A, LU, B, LI, 1.0, indptr, tgt)
    want0, want2 = rk.ranks_by_definition(logit[0])[0], rk.ranks_by_definition(logit[2])[0]
    np.testing.assert_array_equal(ranks, [-1, want0[2], -1, -1, -1, want2[0], -1])
    np.testing.assert_array_equal(np.isnan(scores), ranks < 0)
    np.testing.assert_array_equal(cand, [6, 6, 6])

    monkeypatch.setenv("RFM_CHECK_IDS", "1")
    with pytest.raises(ValueError, match="user id"):
        _abi_ranks(rfm, A, LU, B, LI, 1.0, [0, 1, 2], [0, 1], user_ids=[1, 3])
    with pytest.raises(ValueError, match="target list"):
        _abi_ranks(rfm, A, LU, B, LI, 1.0, indptr, tgt)
    with pytest.raises(ValueError, match="target list"):
        _abi_ranks(rfm, A, LU, B, LI, 1.0, [0, 2, 2, 2], [4, 1])  # not ascending
    with pytest.raises(ValueError, match="target indptr"):
        _abi_ranks(rfm, A, LU, B, LI, 1.0, [0, 2, 1, 2], [1, 4])
    with pytest.raises(ValueError, match="ascending"):
        _abi_ranks(rfm, A, LU, B, LI, 1.0, [0, 1, 1, 1], [1], excl=(np.array([0, 2, 2, 3]), np.array([4, 1, 5])))
    good = (np.array([0, 2, 2, 3]), np.array([1, 4, 5]))
    checked = _abi_ranks(rfm, A, LU, B, LI, 1.0, [0, 3, 3, 5], [0, 1, 1, 2, 5], excl=good)
    monkeypatch.delenv("RFM_CHECK_IDS")
    plain = _abi_ranks(rfm, A, LU, B, LI, 1.0, [0, 3, 3, 5], [0, 1, 1, 2, 5], excl=good)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(checked, plain))
    np.testing.assert_array_equal(plain[2], [4, 6, 5])


def test_methods_reject_bad_arguments(rfm, gold):
    pkg = rfm[0]
    model, sides, _, _ = tgr._fixture_model(rfm, gold, "coat", 16, 0.25)
    for users, items in (([0, NU], [1, 1]), ([-1], [1]), ([0], [NI]), ([0], [-1]), ([0, 1], [1]), ([0.5], [1])):
        with pytest.raises(ValueError):
            model.rank_items(sides, np.array(users), np.array(items))
    E = sp.csr_matrix(rk.heldout(gold[0])[0].astype(np.float64))
    u, i = int(E.nonzero()[0][0]), int(E.nonzero()[1][0])
    with pytest.raises(ValueError, match=rf"pair 1 \(user {u}, item {i}\)"):
        model.rank_items(sides, np.array([0, u]), np.array([int(np.flatnonzero(E[0].toarray().ravel() == 0)[0]), i]), exclude=E)
    with pytest.raises(ValueError):
        model.rank_items(sides, np.array([0]), np.array([1]), exclude=sp.csr_matrix((NU + 1, NI)))
    other = tgr._sides(rfm, gold[0], "kuairec")  # one column wider than the Coat layout
    with pytest.raises(ValueError, match="columns"):
        model.rank_items(other, np.array([0]), np.array([1]))
    empty = model.rank_items(sides, np.zeros(0, np.int64), np.zeros(0, np.int64))
    assert [a.shape for a in empty] == [(0,)] * 3
    fresh = pkg.LogisticMatrixFactorization(estimator="IPS", n_epochs=1, n_factors=24, n_users=NU, n_items=NI,
                                            lr=0.02, reg=0.5, batch_size=1, seed=12345)
    with pytest.raises(AttributeError):
        fresh.rank_items(np.array([0]), np.array([1]))
    mf = tgr._mf_model(pkg, gold[0], 24)
    with pytest.raises(ValueError):
        mf.rank_items(np.array([NU]), np.array([0]))
