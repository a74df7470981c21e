"""Catalogue scoring and top-K on the device through the public Python surface:
``FactorizationMachines.score_pairs`` / ``recommend``, their MF counterparts,
``features.sides_kuairec`` / ``sides_coat``, and the order rule through the C ABI.
Needs an MI355X: ``pytest -m gpu``.  Reference values: ``tests/golden/recommend*.npz``, the
REFERENCE's ``predict()`` over the materialised rows of all 61 x 203 pairs.  Tolerances are those
of ``tests/test_gpu_parity.py``, unchanged."""
import numpy as np
import pytest
from scipy import sparse as sp

import recommend_common as rc
from conftest import assert_elementwise, load_golden, rel_err
from relevance_factorizationmachine_amd import synth

pytestmark = pytest.mark.gpu

_case, fm_parameters = rc.case_name, rc.fm_parameters

CONTRACT = 1e-5
TIGHT = 1e-9
ATOL = 1e-12  # of assert_elementwise
NU, NI = rc.N_USERS, rc.N_ITEMS
SUBSET = np.array([5, 60, 0, 5, 17, 33, 5])  # not monotone, one id three times


@pytest.fixture(scope="module")
def rfm():
    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import features, recommend, runtime
    return pkg, features, recommend, runtime.Runtime.get()


@pytest.fixture(scope="module")
def gold():
    return load_golden("recommend"), {layout: load_golden(f"recommend_fm_{layout}") for layout in rc.LAYOUTS}


def _tables(g):
    return sp.csr_matrix(g["user_table"]), sp.csr_matrix(g["item_table"]), sp.csr_matrix(g["context"])


def _sides(rfm, g, layout):
    _, features, _, rt = rfm
    user, item, ctx = _tables(g)
    if layout == "kuairec":
        return features.sides_kuairec(rt, NU, NI, ctx, user, item)
    return features.sides_coat(rt, user, item)


def _fm_model(pkg, n_features, k, alpha, w0, w, V):
    m = pkg.FactorizationMachines(estimator="IPS", n_epochs=1, n_factors=k, n_features=n_features, lr=1e-4,
                                  batch_size=1, seed=12345, alpha=alpha)
    m.w0.set(np.asarray(w0))
    m.w.set(np.asarray(w))
    m.V.set(np.asarray(V))
    return m


def _fixture_model(rfm, gold, layout, k, alpha):
    g, gls = gold
    w0, w, V = fm_parameters(g, gls[layout], layout, k, alpha)
    sides = _sides(rfm, g, layout)
    return _fm_model(rfm[0], sides.n_features, k, alpha, w0, w, V), sides, gls[layout][f"{_case(k, alpha)}_R"], (w0, w, V)


def _mf_model(pkg, g, k):
    m = pkg.LogisticMatrixFactorization(estimator="IPS", n_epochs=1, n_factors=k, n_users=NU, n_items=NI, lr=0.02,
                                        reg=0.5, batch_size=1, seed=12345)
    m.P.set(g[f"mf_k{k}_P"])
    m.Q.set(g[f"mf_k{k}_Q"])
    m.b_u.set(g[f"mf_k{k}_bu"])
    m.b_i.set(g[f"mf_k{k}_bi"])
    m.b = float(g[f"mf_k{k}_b"])
    return m


def _close(got, want, what):
    print(what, "rel_err", rel_err(got, want))
    assert rel_err(got, want) < TIGHT, (what, rel_err(got, want))
    assert_elementwise(got, want, rtol=CONTRACT, what=what)


def _check_topk_against_scores(items, scores, R, K, what):
    """Forms (a), (b), (c): the returned scores are R's, R along the returned items does not
    increase, and no item left out beats the last one kept -- each within the contract tolerance."""
    assert items.shape == scores.shape == (R.shape[0], K) and items.dtype == np.int32 and scores.dtype == np.float64
    assert (items >= 0).all() and (items < R.shape[1]).all(), what
    picked = np.take_along_axis(R, items.astype(np.int64), axis=1)
    _close(scores, picked, what + " (a)")
    slack = CONTRACT * np.abs(picked) + ATOL
    assert (picked[:, 1:] <= picked[:, :-1] + slack[:, :-1]).all(), what + " (b)"
    for u in range(R.shape[0]):
        assert len(set(items[u].tolist())) == K, (what, u, "an item returned twice")
        rest = np.delete(R[u], items[u])
        if rest.size:
            assert rest.max() <= picked[u, -1] + slack[u, -1], (what, "(c)", u, rest.max(), picked[u, -1])


# --------------------------------------------------------------------------- 1
@pytest.mark.parametrize("layout", rc.LAYOUTS)
@pytest.mark.parametrize("k,alpha", rc.FM_CASES)
def test_fm_score_pairs_matches_reference(rfm, gold, layout, k, alpha):
    model, sides, R, _ = _fixture_model(rfm, gold, layout, k, alpha)
    S = model.score_pairs(sides)
    assert S.shape == (NU, NI) and S.dtype == np.float64
    _close(S, R, f"{layout} {_case(k, alpha)}")
    _close(model.score_pairs(sides, users=SUBSET), R[SUBSET], f"{layout} {_case(k, alpha)} subset")
    np.testing.assert_array_equal(model.score_pairs(sides), S)  # same inputs, same bits


@pytest.mark.parametrize("k", rc.MF_FACTORS)
def test_mf_score_pairs_matches_reference(rfm, gold, k):
    g = gold[0]
    model = _mf_model(rfm[0], g, k)
    _close(model.score_pairs(), g[f"mf_k{k}_R"], f"mf k={k}")
    _close(model.score_pairs(users=SUBSET), g[f"mf_k{k}_R"][SUBSET], f"mf k={k} subset")


# --------------------------------------------------------------------------- 2
def _kuairec_tables(rng, nu, ni):
    """Side tables shaped like the synthetic KuaiRec log's (synth.py): seven one-hot user groups;
    four item reals and one of 31 tags; one context value per user."""
    user = np.hstack([np.eye(s)[rng.integers(0, s, size=nu)] for s in synth.KUAIREC_USER_GROUPS])
    item = np.hstack([rng.standard_normal((ni, 4)), np.eye(synth.KUAIREC_N_TAGS)[rng.integers(0, synth.KUAIREC_N_TAGS, size=ni)]])
    return sp.csr_matrix(user), sp.csr_matrix(item), sp.csr_matrix(rng.standard_normal((nu, 1)))


@pytest.mark.parametrize("k,alpha", [(32, 2.0), (400, 0.25)])
def test_fm_score_pairs_matches_predict_at_catalogue_size(rfm, k, alpha):
    pkg, features, _, rt = rfm
    sh = synth.SHAPES["kuairec_small"]
    nu, ni = sh.n_users, sh.n_items
    user, item, ctx = _kuairec_tables(np.random.default_rng(k), nu, ni)
    sides = features.sides_kuairec(rt, nu, ni, ctx, user, item)
    assert sides.n_features == synth.n_features_of(sh)
    model = pkg.FactorizationMachines(estimator="IPS", n_epochs=1, n_factors=k, n_features=sides.n_features,
                                      lr=1e-4, batch_size=1, seed=7, alpha=alpha)
    uu, ii = rc.all_pairs(nu, ni)
    X = features.fm_features_kuairec(rt, uu, ii, nu, ni, features.take_rows(rt, ctx, uu), user, item)
    want = model.predict(X).reshape(nu, ni)
    del X
    S = model.score_pairs(sides)
    _close(S, want, f"catalogue k={k}")
    # top-K at a size where a workgroup walks several tiles, under two different cuts of the items
    # into splits (the user list three times over makes 67 user tiles instead of 23, and the
    # number of splits goes by the number of user tiles): the order is total, so the lists agree
    for K in (9, 64):
        items, scores = model.recommend(sides, k=K)
        _check_topk_against_scores(items, scores, want, K, f"catalogue k={k} K={K}")
        items3, scores3 = model.recommend(sides, k=K, users=np.tile(np.arange(nu), 3))
        np.testing.assert_array_equal(items3, np.tile(items, (3, 1)))
        np.testing.assert_array_equal(scores3, np.tile(scores, (3, 1)))


# --------------------------------------------------------------------------- 3
@pytest.mark.parametrize("layout", rc.LAYOUTS)
def test_sides_add_up_to_the_assembled_pair_rows(rfm, gold, layout):
    _, features, _, rt = rfm
    g = gold[0]
    user, item, ctx = _tables(g)
    sides = _sides(rfm, g, layout)
    XU, XI = (X.to_scipy() for X in sides.device(rt))
    uu, ii = rc.all_pairs(NU, NI)
    if layout == "kuairec":
        want = features.fm_features_kuairec(rt, uu, ii, NU, NI, ctx[uu], user, item).to_scipy()
    else:
        want = features.fm_features_coat(rt, uu, ii, user, item).to_scipy()
    got = rc.pair_rows(XU, XI, uu, ii)
    want.sort_indices()
    assert got.shape == want.shape
    np.testing.assert_array_equal(got.indptr, want.indptr)
    np.testing.assert_array_equal(got.indices, want.indices)
    np.testing.assert_array_equal(got.data, want.data)  # bit for bit
    # ... and they are the host statement of the layout
    hU, hI = rc.side_matrices(layout, g["user_table"], g["item_table"], g["context"])
    assert abs(XU - hU).nnz == 0 and abs(XI - hI).nnz == 0


# --------------------------------------------------------------------------- 4
@pytest.mark.parametrize("K", [1, 9, 64])
@pytest.mark.parametrize("layout", rc.LAYOUTS)
@pytest.mark.parametrize("k,alpha", rc.FM_CASES)
def test_fm_recommend_matches_reference(rfm, gold, layout, k, alpha, K):
    model, sides, R, _ = _fixture_model(rfm, gold, layout, k, alpha)
    items, scores = model.recommend(sides, k=K)
    _check_topk_against_scores(items, scores, R, K, f"{layout} {_case(k, alpha)} K={K}")
    sub_items, sub_scores = model.recommend(sides, k=K, users=SUBSET)
    np.testing.assert_array_equal(sub_items, items[SUBSET])
    np.testing.assert_array_equal(sub_scores, scores[SUBSET])
    if alpha == 0.25:
        # the reference's probabilities are well separated here (checked, so that the exact
        # comparison cannot silently become a coin toss): the ranking is the reference's exactly
        top = np.sort(R, axis=1)[:, ::-1][:, :11]
        gap = float(np.min(top[:, :-1] - top[:, 1:]))
        print("smallest gap inside the top 10:", gap)
        assert gap > 1e3 * TIGHT, gap
        # ... and down to the ranks compared here: the identity differs from the reference by
        # 1e-14 norm-wise (test_recommend_host.py prints it), a hundred times that keeps order
        deep = np.sort(R, axis=1)[:, ::-1][:, : K + 1]
        assert float(np.min(deep[:, :-1] - deep[:, 1:])) > 1e-12
        want =np.argsort(R, axis=1, kind="stable")[:, ::-1][:, :K]
        np.testing.assert_array_equal(items, want)


# --------------------------------------------------------------------------- 5
def _abi_topk(rfm, A, LU, B, LI, c, K, user_ids=None, excl=None):
    _, _, recommend, rt = rfm
    import torch
    kf = A.shape[1]
    dA, dB = recommend.padded(rt, rt.upload(A), kf), recommend.padded(rt, rt.upload(B), kf)
    dLU, dLI, dc = rt.upload(LU), rt.upload(LI), rt.upload(np.array([c], dtype=np.float64))
    ids = None if user_ids is None else rt.upload(np.asarray(user_ids, dtype=np.int32))
    n_sel = A.shape[0] if user_ids is None else len(user_ids)
    ws = rt.empty((recommend.topk_workspace_bytes(n_sel, B.shape[0], K),), torch.uint8)
    items, scores = rt.empty((n_sel, K), torch.int32), rt.empty((n_sel, K), torch.float64)
    ex = (None, None) if excl is None else (rt.upload(excl[0].astype(np.int64)), rt.upload(excl[1].astype(np.int32)))
    rc_ = rt.lib.rfm_pair_topk(rt.ctx, dA.data_ptr(), dLU.data_ptr(), A.shape[0],
                               None if ids is None else ids.data_ptr(), n_sel, dB.data_ptr(), dLI.data_ptr(),
                               B.shape[0], kf, dc.data_ptr(), None if ex[0] is None else ex[0].data_ptr(),
                               None if ex[1] is None else ex[1].data_ptr(), K, ws.data_ptr(), items.data_ptr(),
                               scores.data_ptr())
    from relevance_factorizationmachine_amd import _lib
    _lib.check(rc_)
    rt.sync()
    return items.cpu().numpy(), scores.cpu().numpy()


def _expect_topk(logit, K):
    items = np.full((logit.shape[0], K), -1, dtype=np.int32)
    scores = np.full((logit.shape[0], K), np.nan)
    for u in range(logit.shape[0]):
        top = rc.stable_topk(logit[u], K)
        items[u, : len(top)] = top
        scores[u, : len(top)] = rc.sigmoid(logit[u, top])
    return items, scores


@pytest.mark.parametrize("n_users,n_items,kf", [(70, 150, 6), (3, 5, 4), (130, 64, 5), (64, 321, 9)])
@pytest.mark.parametrize("K", [1, 9, 64])
def test_order_rule_and_determinism_through_the_abi(rfm, n_users, n_items, kf, K):
    rng = np.random.default_rng(n_users * 1000 + n_items)
    # small integers: every product and sum is exact, and many logits are exactly equal
    A = rng.integers(-2, 3, size=(n_users, kf)).astype(np.float64)
    B = rng.integers(-2, 3, size=(n_items, kf)).astype(np.float64)
    LU = rng.integers(-1, 2, size=n_users).astype(np.float64)
    LI = rng.integers(-1, 2, size=n_items).astype(np.float64)
    A[1] = 0.0     # an all-equal user: every logit is c + LU[1]
    LI[:] = np.where(rng.random(n_items) < 0.5, 0.0, LI)
    B[n_items // 2] = np.nan  # an item that is never ranked
    c = 3.0
    logit = c + LU[:, None] + LI[None, :] + A @ B.T
    logit[:, n_items // 2] = np.nan
    if n_items >= 64:
        assert (np.diff(np.sort(logit[0][~np.isnan(logit[0])])) == 0).any()  # ties exist
    want_items, want_scores = _expect_topk(logit, K)
    items, scores = _abi_topk(rfm, A, LU, B, LI, c, K)
    np.testing.assert_array_equal(items, want_items)
    np.testing.assert_array_equal(np.isnan(scores), want_items < 0)
    ok = want_items >= 0
    _close(scores[ok], want_scores[ok], "abi scores")
    again = _abi_topk(rfm, A, LU, B, LI, c, K)
    np.testing.assert_array_equal(items, again[0])
    assert scores.tobytes() == again[1].tobytes()  # identical bits, NaN padding included
    if n_items - 1 < K:
        assert (items[:, n_items - 1:] == -1).all() and np.isnan(scores[:, n_items - 1:]).all()


def test_abi_rejects_bad_arguments(rfm):
    A, B = np.ones((3, 4)), np.ones((5, 4))
    for K in (0, 65):
        with pytest.raises(ValueError, match="outside 1..64"):
            _abi_topk(rfm, A, np.zeros(3), B, np.zeros(5), 0.0, K, user_ids=[0, 1])


def test_ids_outside_their_tables(rfm, monkeypatch):
    """Never read out of bounds: a user id outside the table scores NaN / ranks nothing, a column
    outside V is skipped; with RFM_CHECK_IDS=1 both, and an unsorted exclusion list, are errors."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    _, _, recommend, rt = rfm
    rng = np.random.default_rng(5)
    A, B = rng.integers(-2, 3, size=(3, 4)).astype(np.float64), rng.integers(-2, 3, size=(6, 4)).astype(np.float64)
    LU, LI = np.zeros(3), np.arange(6.0)
    logit = 1.0 + LI[None, :] + A @ B.T
    good = (np.array([0, 2, 2, 3]), np.array([1, 4, 5]))
    unsorted = (np.array([0, 2, 2, 3]), np.array([4, 1, 5]))

    def side_sums(indices):
        X = sp.csr_matrix((np.ones(3), np.array(indices), np.array([0, 2, 3])), shape=(2, 100))
        dX = rt.upload(X.indptr.astype(np.int64)), rt.upload(X.indices.astype(np.int32)), rt.upload(X.data)
        w, V = rt.upload(np.arange(5.0)), rt.upload(np.arange(15.0).reshape(5, 3))
        dA, dL = rt.empty((2, 4), torch.float64), rt.empty((2,), torch.float64)
        _lib.check(rt.lib.rfm_fm_side_sums(rt.ctx, dX[0].data_ptr(), dX[1].data_ptr(), dX[2].data_ptr(), 2,
                                           w.data_ptr(), V.data_ptr(), 5, 3, dA.data_ptr(), dL.data_ptr()))
        rt.sync()
        return dA.cpu().numpy(), dL.cpu().numpy()

    monkeypatch.delenv("RFM_CHECK_IDS", raising=False)
    items, scores = _abi_topk(rfm, A, LU, B, LI, 1.0, 2, user_ids=[1, 3, -1, 0])
    np.testing.assert_array_equal(items, np.stack([rc.stable_topk(logit[1], 2), [-1, -1], [-1, -1],
                                                   rc.stable_topk(logit[0], 2)]))
    assert np.isnan(scores[1:3]).all() and not np.isnan(scores[[0, 3]]).any()
    dA, dL = side_sums([1, 77, 4])  # column 77 of 5: skipped
    V = np.arange(15.0).reshape(5, 3)
    np.testing.assert_array_equal(dA, np.array([[*V[1], 0.0], [*V[4], 0.0]]))
    np.testing.assert_array_equal(dL, [1.0, 4.0])

    monkeypatch.setenv("RFM_CHECK_IDS", "1")
    with pytest.raises(ValueError, match="user id"):
        _abi_topk(rfm, A, LU, B, LI, 1.0, 2, user_ids=[1, 3])
    with pytest.raises(ValueError, match="ascending"):
        _abi_topk(rfm, A, LU, B, LI, 1.0, 2, excl=unsorted)
    with pytest.raises(ValueError, match="column index"):
        side_sums([1, 77, 4])
    checked = _abi_topk(rfm, A, LU, B, LI, 1.0, 2, excl=good)
    monkeypatch.delenv("RFM_CHECK_IDS")
    plain = _abi_topk(rfm, A, LU, B, LI, 1.0, 2, excl=good)
    np.testing.assert_array_equal(checked[0], plain[0])
    masked = logit.copy()
    masked[0, 1] = masked[0, 4] = masked[2, 5] = np.nan  # user 0: items 1, 4; user 2: item 5
    np.testing.assert_array_equal(plain[0], _expect_topk(masked, 2)[0])


# --------------------------------------------------------------------------- 6
@pytest.mark.parametrize("layout", rc.LAYOUTS)
@pytest.mark.parametrize("K", [1, 9, 64])
def test_saturated_probabilities_are_ranked_by_logit(rfm, gold, layout, K):
    model, sides, R, (w0, w, V) = _fixture_model(rfm, gold, layout, 16, 2.0)
    saturated = float(np.mean((R == 0.0) | (R == 1.0)))
    print("saturated share:", saturated)
    assert saturated > 0.02  # the case is what it is meant to be: probabilities tie, logits do not
    g = gold[0]
    logit = rc.fm_logits(*rc.side_matrices(layout, g["user_table"], g["item_table"], g["context"]), w0, w, V)
    tol = 1e-9 * float(np.max(np.abs(logit)))
    items, scores = model.recommend(sides, k=K)
    _check_topk_against_scores(items, scores, R, K, f"saturated {layout} K={K}")
    exact = 0
    for u in range(NU):
        order = np.argsort(logit[u], kind="stable")[::-1]
        s = logit[u][order]
        for r in range(K):
            apart = (r == 0 or s[r - 1] - s[r] > tol) and (r + 1 >= NI or s[r] - s[r + 1] > tol)
            if apart:
                exact += 1
                assert items[u, r] == order[r], (u, r)
        rest = np.delete(logit[u], items[u])
        assert rest.max() <= logit[u, items[u, -1]] + tol, (u, "(c) on the logit")
    assert exact > 0.9 * NU * K  # the exact form covered (nearly) every rank


# --------------------------------------------------------------------------- 7
@pytest.mark.parametrize("K", [9, 64])
def test_exclusions(rfm, gold, K):
    layout, k, alpha = "kuairec", 33, 0.25
    model, sides, R, (w0, w, V) = _fixture_model(rfm, gold, layout, k, alpha)
    g = gold[0]
    rng = np.random.default_rng(11)
    M = rng.random((NU, NI)) < 0.3
    M[np.arange(NU), model.recommend(sides, k=K)[0][:, 0]] = True  # everybody's best item
    M[4] = True
    M[4, [3, 77, 150]] = False    # user 4 keeps three items: fewer than K
    M[9] = True                   # user 9 keeps none
    M[12] = False                 # user 12 excludes nothing
    E = sp.csr_matrix(M.astype(np.float64))
    logit = rc.fm_logits(*rc.side_matrices(layout, g["user_table"], g["item_table"], g["context"]), w0, w, V)
    masked = logit.copy()
    masked[E.toarray() != 0] = np.nan
    want_items, want_scores = _expect_topk(masked, K)
    for exclude in (E, (E.indptr, E.indices)):
        items, scores = model.recommend(sides, k=K, exclude=exclude)
        np.testing.assert_array_equal(items, want_items)
        for u in range(NU):
            assert not set(items[u][items[u] >= 0].tolist()) & set(E[u].indices.tolist()), u
        ok = want_items >= 0
        np.testing.assert_array_equal(np.isnan(scores), ~ok)
        _close(scores[ok], want_scores[ok], "scores under exclusion")
    assert (want_items[4] >= 0).sum() == 3 and (want_items[9] == -1).all() and (want_items[12] >= 0).all()
    sub = model.recommend(sides, k=K, users=SUBSET, exclude=E)
    np.testing.assert_array_equal(sub[0], want_items[SUBSET])  # the lists go by user id
    with pytest.raises(ValueError):
        model.recommend(sides, k=K, exclude=(E.indptr, E.indices[::-1].copy()))
    with pytest.raises(ValueError):
        model.recommend(sides, k=K, exclude=sp.csr_matrix((NU + 1, NI)))


def test_recommend_rejects_bad_arguments(rfm, gold):
    model, sides, _, _ = _fixture_model(rfm, gold, "coat", 16, 0.25)
    for K in (0, 65):
        with pytest.raises(ValueError, match="outside 1..64"):
            model.recommend(sides, k=K)
    with pytest.raises(ValueError):
        model.recommend(sides, k=3, users=[0, NU])
    with pytest.raises(ValueError):
        model.score_pairs(sides, users=[-1])
    other = _sides(rfm, gold[0], "kuairec")  # one column wider than the Coat layout
    with pytest.raises(ValueError, match="columns"):
        model.score_pairs(other)


# --------------------------------------------------------------------------- 8
@pytest.mark.parametrize("k", rc.MF_FACTORS)
def test_mf_recommend_and_score_pairs_match_predict(rfm, gold, k):
    pkg = rfm[0]
    g = gold[0]
    fresh = pkg.LogisticMatrixFactorization(estimator="IPS", n_epochs=1, n_factors=k, n_users=NU, n_items=NI,
                                            lr=0.02, reg=0.5, batch_size=1, seed=12345)
    with pytest.raises(AttributeError):
        fresh.recommend(k=3)
    with pytest.raises(AttributeError):
        fresh.score_pairs()
    model = _mf_model(pkg, g, k)
    uu, ii = rc.all_pairs(NU, NI)
    want = model.predict(np.stack([uu, ii], axis=1)).reshape(NU, NI)
    _close(model.score_pairs(), want, f"mf k={k} vs predict")
    logit = rc.mf_logits(g[f"mf_k{k}_P"], g[f"mf_k{k}_Q"], g[f"mf_k{k}_bu"], g[f"mf_k{k}_bi"], float(g[f"mf_k{k}_b"]))
    for K in (1, 9, 64):
        items, scores = model.recommend(k=K)
        _check_topk_against_scores(items, scores, want, K, f"mf k={k} K={K}")
        _check_topk_against_scores(items, scores, g[f"mf_k{k}_R"], K, f"mf k={k} K={K} vs reference")
        s = np.sort(logit, axis=1)[:, ::-1][:, : K + 1]
        if np.min(s[:, :-1] - s[:, 1:]) > 1e-9 * np.max(np.abs(logit)):
            np.testing.assert_array_equal(items, _expect_topk(logit, K)[0])
