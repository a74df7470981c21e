"""Deep ranking of the catalogue on the device: ``rank_catalogue`` of
``FactorizationMachines`` / ``LogisticMatrixFactorization``, ``evaluate.CatalogueExposure`` and
``rfm_pair_order`` through the C ABI.  Needs an MI355X: ``pytest -m gpu``.  Items, counts and the
agreement with ``recommend()`` / ``rank_items()`` are compared EXACTLY; the fixture is that of
``test_gpu_recommend.py`` (``tests/golden/recommend*.npz``)."""
import numpy as np
import pytest
from scipy import sparse as sp

import rank_catalogue_common as rcc
import rank_items_common as rk
import recommend_common as rc
import test_gpu_recommend as tgr

pytestmark = pytest.mark.gpu

NU, NI = rcc.NU, rcc.NI
SUBSET = tgr.SUBSET


@pytest.fixture(scope="module")
def rfm():
    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import features, recommend, runtime
    return pkg, features, recommend, runtime.Runtime.get()


@pytest.fixture(scope="module")
def models(rfm):
    """``model -> (rank_catalogue, recommend, rank_items, evaluate)`` of a fixture model, each with
    the sides bound; a device model is set up once and shared."""
    made = {}

    def get(model):
        if model not in made:
            kind, layout, k, alpha = model
            if kind == "mf":
                m, sides = tgr._mf_model(rfm[0], rcc.gold()[0], k), None
            else:
                sides = tgr._sides(rfm, rcc.gold()[0], layout)
                m = tgr._fm_model(rfm[0], sides.n_features, k, alpha, *rcc.fm_parameters(layout, k, alpha))
            bind = (lambda f: f) if sides is None else (lambda f: (lambda *a, **kw: f(sides, *a, **kw)))
            made[model] = (bind(m.rank_catalogue), bind(m.recommend), bind(m.rank_items),
                           lambda ev: ev.evaluate(m, sides))
        return made[model]

    return get


def _abi_order(rfm, A, LU, B, LI, c, depth, user_ids=None, excl=None, workspace_bytes=None, raw=None):
    _, _, recommend, rt = rfm
    import torch
    from relevance_factorizationmachine_amd import _lib
    kf = A.shape[1]
    dA, dB = recommend.padded(rt, rt.upload(A), kf), recommend.padded(rt, rt.upload(B), kf)
    dLU, dLI, dc = rt.upload(LU), rt.upload(LI), rt.upload(np.array([c], dtype=np.float64))
    ids = None if user_ids is None else rt.upload(np.asarray(user_ids, dtype=np.int32))
    n_sel = A.shape[0] if user_ids is None else len(user_ids)
    if workspace_bytes is None:
        workspace_bytes = recommend.order_workspace_bytes(n_sel, B.shape[0], max(int(depth), 1))[1]
    ws = rt.empty((workspace_bytes,), torch.uint8)
    cols = max(int(depth), 1)
    items, scores = rt.empty((n_sel, cols), torch.int32), rt.empty((n_sel, cols), torch.float64)
    n_ranked = rt.empty((n_sel,), torch.int32)
    ex = (None, None) if excl is None else (rt.upload(excl[0].astype(np.int64)),
                                            rt.upload(excl[1].astype(np.int32) if len(excl[1]) else np.zeros(1, np.int32)))
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    args = dict(ctx=rt.ctx, A=dA.data_ptr(), LU=dLU.data_ptr(), n_users=A.shape[0], ids=ptr(ids), n_sel=n_sel,
                B=dB.data_ptr(), LI=dLI.data_ptr(), n_items=B.shape[0], kf=kf, c=dc.data_ptr(), ei=ptr(ex[0]),
                ex=ptr(ex[1]), depth=int(depth), ws=ws.data_ptr(), ws_bytes=int(workspace_bytes),
                items=items.data_ptr(), scores=scores.data_ptr(), n_ranked=n_ranked.data_ptr())
    args.update(raw or {})
    _lib.check(rt.lib.rfm_pair_order(*args.values()))
    rt.sync()
    return items.cpu().numpy(), scores.cpu().numpy(), n_ranked.cpu().numpy()


def _check(got, want, what):
    """``got`` of the device against ``rcc.expected_lists``: items, padding and counts exactly, the
    scores = sigmoid of the expected logits at 1e-15 relative (two roundings of a double)."""
    items, scores, n_ranked = got
    w_items, w_logits, w_n = want
    assert items.dtype == np.int32 and scores.dtype == np.float64 and n_ranked.dtype == np.int32
    np.testing.assert_array_equal(items, w_items, err_msg=what)
    np.testing.assert_array_equal(n_ranked, w_n, err_msg=what)
    np.testing.assert_array_equal(np.isnan(scores), w_items < 0, err_msg=what)  # padding: -1 / NaN
    ok = w_items >= 0
    if ok.any():
        w_scores = rc.sigmoid(w_logits[ok])
        err = float(np.max(np.abs(scores[ok] - w_scores) / w_scores))
        print(what, "largest relative error of a score:", err)
        assert err <= 1e-15, (what, err)


# --------------------------------------------------------------------------- 1
SHAPES = [(3, 1, 1), (5, 63, 4), (70, 64, 5), (64, 65, 8), (2, 8197, 4)]
PATTERNS = ["three_values", "all_equal", "rising", "falling", "nan_items", "nan_user", "inf_items"]


def _pattern_operands(pattern, n_users, n_items, kf):
    """Integer-valued operands (every product and sum is exact, ties are real) and their logits."""
    rng = np.random.default_rng(n_users * 1000 + n_items)
    A, B = np.zeros((n_users, kf)), rng.integers(-2, 3, size=(n_items, kf)).astype(np.float64)
    LU, LI = rng.integers(-1, 2, size=n_users).astype(np.float64), np.zeros(n_items)
    if pattern == "three_values":
        A[:, 0] = 1.0
        B[:, 0] = rng.integers(-1, 2, size=n_items)
    elif pattern == "all_equal":
        pass  # A = 0: every logit of a user is c + LU[u]
    elif pattern in ("rising", "falling"):
        sign = 1.0 if pattern == "rising" else -1.0
        A[:, 0] = sign
        B[:, 0] = np.arange(n_items)
        LI[:] = sign * np.arange(n_items)
    else:  # many ties among a few integer values, through every factor
        A = rng.integers(-2, 3, size=(n_users, kf)).astype(np.float64)
        LI = rng.integers(-1, 2, size=n_items).astype(np.float64)
        if pattern == "nan_items":
            LI[rng.random(n_items) < 0.2] = np.nan
            LI[n_items // 2] = np.nan
        elif pattern == "nan_user":
            LU[1 % n_users] = np.nan
        else:
            LI[n_items // 3] = np.inf
            if n_items > 1:
                LI[(n_items // 3 + 1 + n_items // 2) % n_items] = -np.inf
    c = 3.0
    with np.errstate(invalid="ignore"):
        logit = c + LU[:, None] + LI[None, :] + A @ B.T
    return A, LU, B, LI, c, logit


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n_users,n_items,kf", SHAPES)
def test_order_rule_through_the_abi(rfm, n_users, n_items, kf, pattern):
    A, LU, B, LI, c, logit = _pattern_operands(pattern, n_users, n_items, kf)
    depths = [1, 64, 65, 128, 129, n_items, n_items + 7]
    if n_items == 8197:
        depths += [4096, 4097, 8197]  # up to three pages
    for depth in sorted(set(depths)):
        want = rcc.expected_lists(logit, depth)
        _check(_abi_order(rfm, A, LU, B, LI, c, depth), want, f"{pattern} {n_users}x{n_items} depth {depth}")
    full = want[0]  # the deepest call (at least n_items + 7): the whole order, then padding
    assert (full[:, n_items:] == -1).all()
    if pattern == "all_equal":
        np.testing.assert_array_equal(full[:, :n_items], np.tile(np.arange(n_items)[::-1], (n_users, 1)))
    elif pattern == "rising":
        np.testing.assert_array_equal(full[:, :n_items], np.tile(np.arange(n_items)[::-1], (n_users, 1)))
    elif pattern == "falling":
        np.testing.assert_array_equal(full[:, :n_items], np.tile(np.arange(n_items), (n_users, 1)))
    elif pattern == "nan_items":
        assert np.isnan(LI).any() and not np.isin(full, np.flatnonzero(np.isnan(LI))).any()
        assert (want[2] == n_items - np.isnan(LI).sum()).all()
    elif pattern == "nan_user":
        assert want[2][1 % n_users] == 0 and (full[1 % n_users] == -1).all()
        assert (np.delete(want[2], 1 % n_users) == n_items).all()
    elif pattern == "inf_items":
        assert (full[:, 0] == n_items // 3).all() and (want[2] == n_items).all()
        if n_items > 1:
            assert (full[:, n_items - 1] == (n_items // 3 + 1 + n_items // 2) % n_items).all()
    elif n_items >= 63:
        assert (np.diff(logit[0][full[0, :n_items]]) == 0).any()  # three values: ties are real


# --------------------------------------------------------------------------- 2
def test_exclusion_lists_and_user_subsets_through_the_abi(rfm):
    n_users, n_items, kf = 70, 150, 6
    A, LU, B, LI, c, logit = _pattern_operands("nan_items", n_users, n_items, kf)
    rng = np.random.default_rng(8)
    M = rng.random((n_users, n_items)) < 0.3
    M[0] = False             # an empty list
    M[n_users - 1] = True    # a list naming every item
    E = sp.csr_matrix(M.astype(np.float64))
    excl = (E.indptr, E.indices)
    sel = np.concatenate([[n_users - 1, 0, 33, 0], rng.integers(0, n_users, size=n_users + 3)])  # not ascending, repeats
    for depth in (9, 64, 150, 200):
        got = _abi_order(rfm, A, LU, B, LI, c, depth, excl=excl)
        _check(got, rcc.expected_lists(logit, depth, M), f"exclusion lists, depth {depth}")
        assert got[2][0] == (~np.isnan(logit[0])).sum() and got[2][n_users - 1] == 0 and (got[0][n_users - 1] == -1).all()
        sub = _abi_order(rfm, A, LU, B, LI, c, depth, user_ids=sel, excl=excl)
        _check(sub, rcc.expected_lists(logit, depth, M, users=sel), f"exclusion lists and a user list, depth {depth}")
        assert all(a[sel].tobytes() == b.tobytes() for a, b in zip(got, sub))  # the lists go by user id
    # lists that name nothing at all / every item of every user
    none = (np.zeros(n_users + 1, np.int64), np.zeros(0, np.int32))
    _check(_abi_order(rfm, A, LU, B, LI, c, 200, excl=none), rcc.expected_lists(logit, 200), "empty exclusion lists")
    every = sp.csr_matrix(np.ones((n_users, n_items)))
    items, scores, n_ranked = _abi_order(rfm, A, LU, B, LI, c, 70, excl=(every.indptr, every.indices))
    assert (items == -1).all() and np.isnan(scores).all() and (n_ranked == 0).all()


def test_abi_rejects_bad_arguments(rfm):
    _, _, recommend, rt = rfm
    A, B = np.ones((3, 4)), np.ones((5, 4))
    ok = dict(depth=4, user_ids=[0, 1])
    items, _, n_ranked = _abi_order(rfm, A, np.zeros(3), B, np.zeros(5), 0.0, **ok)
    np.testing.assert_array_equal(items, [[4, 3, 2, 1]] * 2)
    np.testing.assert_array_equal(n_ranked, [5, 5])
    least = recommend.order_workspace_bytes(2, 5, 4)[0]
    for raw, match in (({"depth": 0}, "depth"), ({"depth": -5}, "depth"), ({"ws": None}, "null"),
                       ({"items": None}, "null"), ({"scores": None}, "null"), ({"n_ranked": None}, "null"),
                       ({"ws_bytes": least - 1}, "less than one block"), ({"ws_bytes": 0}, "less than one block"),
                       ({"kf": 0}, "n_factors"), ({"A": None}, "null"), ({"ids": None}, "every user is selected"),
                       ({"ei": rt.upload(np.zeros(4, np.int64)).data_ptr()}, "exclusion lists without items"),
                       ({"n_sel": -1}, "n_sel_users")):
        with pytest.raises(ValueError, match=match):
            _abi_order(rfm, A, np.zeros(3), B, np.zeros(5), 0.0, raw=raw, **ok)
    _abi_order(rfm, A, np.zeros(3), B, np.zeros(5), 0.0, raw={"n_sel": 0}, **ok)  # no selected user: nothing to do
    _abi_order(rfm, A, np.zeros(3), B, np.zeros(5), 0.0, workspace_bytes=least, **ok)


def test_methods_take_exclusions_and_subsets_and_reject_bad_arguments(rfm, models):
    pkg, _, recommend, rt = rfm
    M = np.random.default_rng(11).random((NU, NI)) < 0.3
    M[4] = True
    M[4, [3, 77, 150]] = False    # user 4 keeps three items
    M[9] = True                   # user 9 keeps none
    M[12] = False                 # user 12 excludes nothing
    E = sp.csr_matrix(M.astype(np.float64))
    for model in (("fm", "kuairec", 33, 0.25), ("mf", None, 24, None)):
        rank_catalogue = models(model)[0]
        Z = rcc.logits(model)
        assert rk.min_relative_gap(Z) > 1e-9  # the exact comparison below is not a coin toss
        for depth in (5, 100, 210):
            want = rcc.expected_lists(Z, depth, M)
            for exclude in (E, (E.indptr, E.indices)):
                items, scores, n_ranked = rank_catalogue(depth, exclude=exclude)
                np.testing.assert_array_equal(items, want[0])
                np.testing.assert_array_equal(n_ranked, want[2])
                np.testing.assert_array_equal(np.isnan(scores), want[0] < 0)
                tgr._close(scores[want[0] >= 0], rc.sigmoid(want[1][want[0] >= 0]), f"{rk.model_id(model)} scores")
            assert n_ranked[4] == 3 and n_ranked[9] == 0 and n_ranked[12] == NI
            sub = rank_catalogue(depth, users=SUBSET, exclude=E)
            assert all(a[SUBSET].tobytes() == b.tobytes() for a, b in zip((items, scores, n_ranked), sub))
        empty = rank_catalogue(7, users=np.zeros(0, np.int64))
        assert [a.shape for a in empty] == [(0, 7), (0, 7), (0,)]
        for depth in (0, -1, 2.5, "3", None, True):
            with pytest.raises(ValueError):
                rank_catalogue(depth)
        with pytest.raises(ValueError):
            rank_catalogue(3, users=[0, NU])
        with pytest.raises(ValueError):
            rank_catalogue(3, exclude=(E.indptr, E.indices[::-1].copy()))
        with pytest.raises(ValueError):
            rank_catalogue(3, exclude=sp.csr_matrix((NU + 1, NI)))
    model, sides, _, _ = tgr._fixture_model(rfm, rcc.gold(), "coat", 16, 0.25)
    other = tgr._sides(rfm, rcc.gold()[0], "kuairec")  # one column wider than the Coat layout
    with pytest.raises(ValueError, match="columns"):
        model.rank_catalogue(other, 3)
    fresh = pkg.LogisticMatrixFactorization(estimator="IPS", n_epochs=1, n_factors=24, n_users=NU, n_items=NI,
                                            lr=0.02, reg=0.5, batch_size=1, seed=12345)
    with pytest.raises(AttributeError):
        fresh.rank_catalogue(3)
    operands = recommend.operands(model, sides)
    with pytest.raises(ValueError, match="less than one block"):
        recommend.rank_catalogue(*operands, 5, workspace_bytes=recommend.order_workspace_bytes(NU, NI, 5)[0] - 1)


# --------------------------------------------------------------------------- 3
@pytest.mark.parametrize("model", rcc.MODELS, ids=rcc.model_id)
def test_agreement_with_recommend_and_rank_items(rfm, models, model):
    rank_catalogue, recommend, rank_items, _ = models(model)
    Z, train = rcc.logits(model), rcc.train_mask()
    gap = rk.min_relative_gap(Z)
    print(rk.model_id(model), "smallest relative gap between neighbouring logits of a user:", gap)
    assert gap > 1e-9  # the comparison with the NumPy logits below is not a coin toss
    E = sp.csr_matrix(train.astype(np.float64))
    for exclude, mask in ((None, None), (E, train)):
        what = rk.model_id(model) + (" train pairs excluded" if mask is not None else "")
        items, scores, n_ranked = rank_catalogue(NI, exclude=exclude)
        assert items.shape == scores.shape == (NU, NI) and n_ranked.shape == (NU,)
        assert items.dtype == np.int32 and scores.dtype == np.float64 and n_ranked.dtype == np.int32
        # the first 64 columns are recommend()'s bytes
        top_items, top_scores = recommend(64, exclude=exclude)
        assert np.ascontiguousarray(items[:, :64]).tobytes() == top_items.tobytes(), what
        assert np.ascontiguousarray(scores[:, :64]).tobytes() == top_scores.tobytes(), what
        # rank_items of the r-th returned item is r, with the same score bytes and candidate count
        ok = items >= 0
        rows = np.repeat(np.arange(NU), NI).reshape(NU, NI)
        ranks, rscores, cand = rank_items(rows[ok], items[ok], exclude=exclude)
        np.testing.assert_array_equal(ranks, np.tile(np.arange(NI), (NU, 1))[ok], err_msg=what)
        assert rscores.tobytes() == scores[ok].tobytes(), what
        np.testing.assert_array_equal(cand, n_ranked[rows[ok]], err_msg=what)
        np.testing.assert_array_equal(ok.sum(axis=1), n_ranked, err_msg=what)
        assert np.isnan(scores[~ok]).all() and not np.isnan(scores[ok]).any()
        # ... and the definition on the NumPy logits
        for u in range(NU):
            r, n = rk.ranks_by_definition(Z[u], None if mask is None else mask[u])
            assert n_ranked[u] == n and (items[u, n:] == -1).all(), (what, u)
            np.testing.assert_array_equal(r[items[u, :n]], np.arange(n), err_msg=f"{what} user {u}")
        if mask is not None:
            assert not mask[rows[ok], items[ok]].any()
            np.testing.assert_array_equal(n_ranked, NI - mask.sum(axis=1))
        else:
            np.testing.assert_array_equal(np.sort(items, axis=1), np.tile(np.arange(NI), (NU, 1)))
        tgr._close(scores[ok], rc.sigmoid(Z[rows[ok], items[ok]]), what)


# --------------------------------------------------------------------------- 4
def test_determinism_block_cuts_and_user_subsets(rfm):
    _, _, recommend, rt = rfm
    model, sides, _, _ = tgr._fixture_model(rfm, rcc.gold(), "kuairec", 33, 2.0)
    operands = recommend.operands(model, sides)
    E = sp.csr_matrix(rcc.train_mask().astype(np.float64))
    users = np.tile(np.arange(NU), 4)[:200]
    least, preferred = recommend.order_workspace_bytes(200, NI, NI)
    assert 3 * least < preferred  # 200 users at the minimum: four blocks of 64, 64, 64 and 8

    def call(**kw):
        return recommend.rank_catalogue(*operands, NI, exclude=E, **kw)

    full = call(users=users)
    again = call(users=users)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(full, again))  # the same bits, NaN padding included
    for ws in (least, least + 1, 2 * least, preferred - 1, 4 * preferred):
        cut = call(users=users, workspace_bytes=ws)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(full, cut)), ws
    everyone = call()
    assert all(a[users].tobytes() == b.tobytes() for a, b in zip(everyone, full))
    sub = call(users=SUBSET)
    assert all(a[SUBSET].tobytes() == b.tobytes() for a, b in zip(everyone, sub))
    assert (everyone[0][:, NI - 1] == -1).all() and (everyone[2] < NI).all()


def test_pages_and_blocks_together_through_the_abi(rfm):
    """130 users x 4 300 items to the full depth: two pages per block, and at the least workspace
    three blocks (64, 64 and 2 users); a user list that repeats and is not ascending."""
    _, _, recommend, _ = rfm
    n_users, n_items, kf = 130, 4300, 5
    A, LU, B, LI, c, _ = _pattern_operands("inf_items", n_users, n_items, kf)
    LU[5], LI[7] = np.nan, np.nan  # a user without candidates; the others have 4 299: 203 on the second page
    with np.errstate(invalid="ignore"):
        logit = c + LU[:, None] + LI[None, :] + A @ B.T
    least, preferred = recommend.order_workspace_bytes(n_users, n_items, n_items)
    want = rcc.expected_lists(logit, n_items)
    assert want[2][5] == 0 and (np.delete(want[2], 5) == n_items - 1).all()
    one = _abi_order(rfm, A, LU, B, LI, c, n_items, workspace_bytes=preferred)
    _check(one, want, "one block, two pages")
    cut = _abi_order(rfm, A, LU, B, LI, c, n_items, workspace_bytes=least)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(one, cut))
    sel = np.arange(n_users)[::-1].repeat(2)[:-1]
    sub = _abi_order(rfm, A, LU, B, LI, c, n_items, user_ids=sel, workspace_bytes=2 * least)
    assert all(a[sel].tobytes() == b.tobytes() for a, b in zip(one, sub))


# --------------------------------------------------------------------------- 5
@pytest.mark.parametrize("model", rcc.MODELS, ids=rcc.model_id)
def test_catalogue_exposure_end_to_end(rfm, models, model):
    from relevance_factorizationmachine_amd.evaluate import CatalogueExposure

    evaluate = models(model)[3]
    assert rk.min_relative_gap(rcc.logits(model)) > 1e-9
    ps = rcc.item_pscores()
    E = sp.csr_matrix(rcc.train_mask().astype(np.float64))
    got = evaluate(CatalogueExposure(NI, rcc.K_LIST, rcc.METRICS, item_pscores=ps, exclude=E))
    rcc.assert_exposure_equal(got, rcc.fixture_oracle(model, True), rk.model_id(model))
    assert np.isnan(got["ME"][-1])  # no user has 203 candidates
    got_all = evaluate(CatalogueExposure(NI, rcc.K_LIST, rcc.METRICS, item_pscores=ps))
    rcc.assert_exposure_equal(got_all, rcc.fixture_oracle(model, False), rk.model_id(model) + " no exclusion")
    assert got_all["CatalogCoverage"][-1] == 1.0
    # users=: only they count
    Z = rcc.logits(model)
    sub = evaluate(CatalogueExposure(NI, rcc.K_LIST, rcc.METRICS, item_pscores=ps, exclude=E, users=np.unique(SUBSET)))
    keep = np.zeros(NU, dtype=bool)
    keep[SUBSET] = True
    want = rcc.exposure_oracle(np.where(keep[:, None], Z, np.nan), rcc.train_mask(), ps)
    rcc.assert_exposure_equal(sub, want, rk.model_id(model) + " user subset")


# --------------------------------------------------------------------------- 6
def test_ids_outside_their_tables(rfm, monkeypatch):
    """Never read out of bounds: a user id outside the table gives an all-NaN row (items -1,
    n_ranked 0); with RFM_CHECK_IDS=1 it, and an unsorted exclusion list, are errors."""
    rng = np.random.default_rng(5)
    A, B = rng.integers(-2, 3, size=(3, 4)).astype(np.float64), rng.integers(-2, 3, size=(6, 4)).astype(np.float64)
    LU, LI = np.zeros(3), np.arange(6.0)
    logit = 1.0 + LI[None, :] + A @ B.T
    good = (np.array([0, 2, 2, 3]), np.array([1, 4, 5]))
    unsorted = (np.array([0, 2, 2, 3]), np.array([4, 1, 5]))
    monkeypatch.delenv("RFM_CHECK_IDS", raising=False)
    items, scores, n_ranked = _abi_order(rfm, A, LU, B, LI, 1.0, 8, user_ids=[1, 3, -1, 0])
    want = rcc.expected_lists(logit, 8, users=[1, 0])
    np.testing.assert_array_equal(items[[0, 3]], want[0])
    assert (items[1:3] == -1).all() and np.isnan(scores[1:3]).all()
    np.testing.assert_array_equal(n_ranked, [6, 0, 0, 6])
    # ... also with exclusion lists, which go by user id
    items, _, n_ranked = _abi_order(rfm, A, LU, B, LI, 1.0, 8, user_ids=[1, 3, -1, 0], excl=good)
    np.testing.assert_array_equal(n_ranked, [6, 0, 0, 4])

    monkeypatch.setenv("RFM_CHECK_IDS", "1")
    with pytest.raises(ValueError, match="user id"):
        _abi_order(rfm, A, LU, B, LI, 1.0, 8, user_ids=[1, 3])
    with pytest.raises(ValueError, match="ascending"):
        _abi_order(rfm, A, LU, B, LI, 1.0, 8, excl=unsorted)
    checked = _abi_order(rfm, A, LU, B, LI, 1.0, 8, excl=good)
    monkeypatch.delenv("RFM_CHECK_IDS")
    plain = _abi_order(rfm, A, LU, B, LI, 1.0, 8, excl=good)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(checked, plain))
    masked = logit.copy()
    masked[0, 1] = masked[0, 4] = masked[2, 5] = np.nan  # user 0: items 1, 4; user 2: item 5
    _check(plain, rcc.expected_lists(masked, 8), "checked exclusion lists")
