"""The item -> users direction through the model classes (needs an MI355X: ``pytest -m
gpu``): ``recommend_users`` / ``rank_users`` / ``rank_audience`` of ``LogisticMatrixFactorization`` and
``FactorizationMachines`` against the forward methods of the same model.  The catalogues are the small
ones of the fold-in flows (MF: 9 users x 20 items; FM: a coat-shaped ``Sides`` of 12 users x 9 items),
at most 64 x 64, so that ``recommend(k = n_items)`` and ``recommend_users(k = n_users)`` both return
every pair and the two directions can be compared pair by pair, exactly."""
import numpy as np
import pytest
from scipy import sparse as sp

import audience_common as ac

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from relevance_factorizationmachine_amd import runtime
    return runtime.Runtime.get()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else a.dtype)


def _mf(k=12):
    from test_gpu_fold_in import N_ITEMS, N_OLD, _flow_case, _user_side_model
    model, _ = _user_side_model(_flow_case(k=k))
    return model, (), N_OLD, N_ITEMS


def _fm(k=12):
    import fm_fold_common as fc
    from test_gpu_fm_fold import _flow
    model, sides = _flow(k)[:2]
    return model, (sides,), fc.FLOW_USERS, fc.FLOW_ITEMS


def _matrix(ids, values, n_cols):
    """Lists of every column of a row (ids a permutation per row) -> the dense [rows, n_cols] matrix."""
    assert (np.sort(ids, axis=1) == np.arange(n_cols)).all()
    out = np.empty(ids.shape)
    np.put_along_axis(out, ids.astype(np.int64), values, axis=1)
    return out


# --------------------------------------------------------------------------- direction agreement
@pytest.mark.parametrize("make", [_mf, _fm], ids=["mf", "fm"])
@pytest.mark.parametrize("k", [12, 13])  # the operands as they are, and zero-padded to 16
def test_both_directions_give_one_pair_one_score(rt, make, k):
    model, lead, n_users, n_items = make(k)
    assert n_users <= 64 and n_items <= 64
    items, scores = model.recommend(*lead, n_items)
    S = _matrix(items, scores, n_items)                   # [u, i]
    users, uscores = model.recommend_users(*lead, n_users)
    assert users.shape == (n_items, n_users) and users.dtype == np.int32 and uscores.dtype == np.float64
    T = _matrix(users, uscores, n_users)                  # [i, u]
    assert ac.same_bytes(T, S.T.copy()), "the score of (u, i) and of (i, u) are not the same float64"
    # each direction ranks by its own candidates: the lists are the rankings of S's columns
    logit_order = np.argsort(-T, axis=1, kind="stable")
    distinct = np.array([len(np.unique(row)) == n_users for row in T])
    np.testing.assert_array_equal(users[distinct], logit_order[distinct])
    # rank_users agrees with rank_audience at full depth, and that with recommend_users
    deep, dscores, n_ranked = model.rank_audience(*lead, n_users)
    assert ac.same_bytes(deep, users) and ac.same_bytes(dscores, uscores) and (n_ranked == n_users).all()
    more, _, _ = model.rank_audience(*lead, n_users + 3, workspace_bytes=None)
    assert ac.same_bytes(more[:, :n_users], users) and (more[:, n_users:] == -1).all()
    ii, uu = np.repeat(np.arange(n_items), n_users), np.tile(np.arange(n_users), n_items)
    shuffle = np.random.default_rng(k).permutation(len(ii))
    ranks, rscores, cand = model.rank_users(*lead, ii[shuffle], uu[shuffle])
    assert (cand == n_users).all()
    np.testing.assert_array_equal(deep[ii[shuffle], ranks], uu[shuffle])
    assert ac.same_bytes(rscores, T[ii[shuffle], uu[shuffle]])
    # a selection of items, any order, repeats allowed
    sel = np.array([n_items - 1, 0, 3, 0])
    sub_users, sub_scores = model.recommend_users(*lead, 5, items=sel)
    assert ac.same_bytes(sub_users, users[sel, :5]) and ac.same_bytes(sub_scores, uscores[sel, :5])
    sub_deep, _, sub_n = model.rank_audience(*lead, 4, items=sel)
    assert ac.same_bytes(sub_deep, users[sel, :4]) and (sub_n == n_users).all()


# --------------------------------------------------------------------------- shared exclude
@pytest.mark.parametrize("make", [_mf, _fm], ids=["mf", "fm"])
def test_one_exclude_matrix_excludes_the_same_pairs_in_both_directions(rt, make):
    model, lead, n_users, n_items = make()
    M = np.random.default_rng(n_users).random((n_users, n_items)) < 0.3
    M[2] = True       # a user who is shown nothing ...
    M[:, 4] = True    # ... and an item shown to nobody
    M[5] = False
    M[5, 4] = True
    E = sp.csr_matrix(M.astype(np.float64))
    items, scores = model.recommend(*lead, n_items, exclude=E)
    users, uscores = model.recommend_users(*lead, n_users, exclude=E)
    forward = np.zeros((n_users, n_items), dtype=bool)
    rows, cols = np.nonzero(items >= 0)
    forward[rows, items[rows, cols]] = True
    backward = np.zeros((n_users, n_items), dtype=bool)
    rows, cols = np.nonzero(users >= 0)
    backward[users[rows, cols], rows] = True
    np.testing.assert_array_equal(forward, ~M)
    np.testing.assert_array_equal(backward, ~M)
    assert (users[4] == -1).all() and np.isnan(uscores[4]).all()
    S = np.full((n_users, n_items), np.nan)
    S[np.nonzero(items >= 0)[0], items[items >= 0]] = scores[items >= 0]
    T = np.full((n_items, n_users), np.nan)
    T[np.nonzero(users >= 0)[0], users[users >= 0]] = uscores[users >= 0]
    assert ac.same_bytes(T, S.T.copy())
    # the (indptr, indices) form by user serves both directions too
    lists = (E.indptr.astype(np.int64), E.indices.astype(np.int32))
    again, _ = model.recommend_users(*lead, n_users, exclude=lists)
    assert ac.same_bytes(again, users)
    deep, _, n_ranked = model.rank_audience(*lead, n_users, exclude=E)
    assert ac.same_bytes(deep, users)
    np.testing.assert_array_equal(n_ranked, (~M).sum(axis=0))
    i, u = np.nonzero(~M.T)
    ranks, _, cand = model.rank_users(*lead, i, u, exclude=E)
    np.testing.assert_array_equal(deep[i, ranks], u)
    np.testing.assert_array_equal(cand, (~M).sum(axis=0)[i])
    with pytest.raises(ValueError, match="is in the user's exclusion list"):
        model.rank_users(*lead, [4], [0], exclude=E)


# --------------------------------------------------------------------------- folded items
def _same_lists(a, b, what):
    for name, x, y in zip(("users", "scores", "third"), a, b):
        differ = _bits(x) != _bits(y)
        print(f"{what} {name}: {int(differ.sum())} of {differ.size} elements differ")
    for x, y in zip(a, b):
        assert ac.same_bytes(x, y), what


@pytest.mark.parametrize("k", [12, 13])
def test_mf_folded_items_are_served_as_appended_items_are(rt, k):
    from oracle import cpu_ref
    from test_gpu_fold_in import N_ITEMS, N_OLD, _flow_case, _model
    case = _flow_case("flow-items", n_fixed=N_OLD, k=k)
    F, fb = case.fixed()                                  # the users are the fixed side here
    _, Q, _, bi = cpu_ref.mf_init(13, 1, N_ITEMS, case.k)
    model = _model(N_OLD, N_ITEMS, F, Q, fb, bi)
    folded = model.fold_in_items(case.data("item", True), case.n_new, case.n_passes)
    E = sp.csr_matrix((np.random.default_rng(k).random((N_OLD, case.n_new)) < 0.3).astype(np.float64))
    sel = np.array([3, 0, 3])
    served = [model.recommend_users(5, new_items=folded), model.recommend_users(N_OLD, items=sel, exclude=E, new_items=folded),
              model.rank_audience(N_OLD + 2, new_items=folded),
              model.rank_users(np.arange(case.n_new), np.arange(case.n_new) % N_OLD, new_items=folded)]
    assert served[0][0].shape == (case.n_new, 5)
    for handle, want in ((model.P, F), (model.Q, Q), (model.b_u, fb), (model.b_i, bi)):
        assert ac.same_bytes(handle(), np.asarray(want, dtype=np.float64)), "the model was written"
    assert model.n_items == N_ITEMS
    ids = model.append_items(folded)
    grown_E = sp.hstack([sp.csr_matrix((N_OLD, N_ITEMS)), E]).tocsr()
    after = [model.recommend_users(5, items=ids), model.recommend_users(N_OLD, items=ids[sel], exclude=grown_E),
             model.rank_audience(N_OLD + 2, items=ids), model.rank_users(ids, np.arange(case.n_new) % N_OLD)]
    for a, b, what in zip(served, after, ("recommend_users", "items= and exclude=", "rank_audience", "rank_users")):
        _same_lists(a, b, f"mf k={k} {what}")
    # folded users and folded items together
    users_case = _flow_case(k=k)
    new_users = model.fold_in_users(users_case.data("user", True), users_case.n_new, users_case.n_passes)
    both, _ = model.recommend_users(users_case.n_new, new_items=folded, new_users=new_users)
    assert both.shape == (case.n_new, users_case.n_new) and (np.sort(both, axis=1) == np.arange(users_case.n_new)).all()


@pytest.mark.parametrize("k", [12, 13])
def test_fm_folded_items_are_served_as_appended_columns_are(rt, k):
    """Bit for bit.  ``new_items=`` does not serve the folded operands ``L = l + omega + g . nu`` that
    rfm_fm_fold_in stores (they round otherwise than the side sums of the grown row, by up to 2 ulp of
    a score): the item side comes from one side-sum launch over the grown rows
    (``recommend.grown_side_sums``), the kernel that a ``Sides`` of the grown width goes through."""
    import fm_fold_common as fc
    from relevance_factorizationmachine_amd import recommend as rec
    from test_gpu_fm_fold import _flow
    model, sides, prob, lr, (w0, w, V) = _flow(k, "item")
    n_users, n_new = fc.FLOW_USERS, prob.n_new
    folded = model.fold_in_items(sides, prob.new_rows, prob.data, prob.n_passes, lr=lr)
    E = sp.csr_matrix((np.random.default_rng(k).random((n_users, n_new)) < 0.3).astype(np.float64))
    sel = np.array([3, 0, 3])
    served = [model.recommend_users(sides, 5, new_items=folded),
              model.recommend_users(sides, n_users, items=sel, exclude=E, new_items=folded),
              model.rank_audience(sides, n_users + 2, new_items=folded),
              model.rank_users(sides, np.arange(n_new), np.arange(n_new) % n_users, new_items=folded)]
    assert served[0][0].shape == (n_new, 5)
    sums, _ = rec.grown_side_sums(model._rt, model, folded)
    model._rt.sync()
    assert ac.same_bytes(sums.cpu().numpy(), folded.A.cpu().numpy()), "the grown rows' sums are the folded A"
    into = rec.operands(model, sides, new_items=folded)
    again = rec.operands(model, sides, into=into, new_items=folded)
    assert again.B.data_ptr() == into.B.data_ptr() and tuple(again.B.shape) == (n_new, rec.pad4(k))
    assert ac.same_bytes(rec.topk_users(*again, 5)[1], served[0][1])
    with pytest.raises(ValueError, match="into a buffer of"):
        rec.operands(model, sides, into=rec.operands(model, sides), new_items=folded)
    for handle, want in ((model.V, V), (model.w, w), (model.w0, w0)):
        assert ac.same_bytes(handle(), np.asarray(want, dtype=np.float64).reshape(handle().shape)), "the model was written"
    assert model.n_features == prob.n_features
    model.append_columns(folded)
    grown = rec.Sides(*fc.grown_sides(prob))
    ids = fc.FLOW_ITEMS + np.arange(n_new)
    grown_E = sp.hstack([sp.csr_matrix((n_users, fc.FLOW_ITEMS)), E]).tocsr()
    after = [model.recommend_users(grown, 5, items=ids), model.recommend_users(grown, n_users, items=ids[sel], exclude=grown_E),
             model.rank_audience(grown, n_users + 2, items=ids), model.rank_users(grown, ids, np.arange(n_new) % n_users)]
    for a, b in zip(served, after):  # the figures first: the largest distance of the scores, in units of the last place
        apart = np.abs(a[1] - b[1]) / np.spacing(np.abs(b[1]))
        print(f"fm k={k}: users differ at {int((a[0] != b[0]).sum())} places, scores at most {np.nanmax(apart):.1f} ulp apart")
    for a, b, what in zip(served, after, ("recommend_users", "items= and exclude=", "rank_audience", "rank_users")):
        _same_lists(a, b, f"fm k={k} {what}")


# --------------------------------------------------------------------------- errors
def test_errors_are_those_of_the_forward_counterparts(rt):
    import fm_fold_common as fc
    from test_gpu_fm_fold import _flow
    from test_gpu_fold_in import N_ITEMS, N_OLD, _flow_case, _user_side_model
    case = _flow_case()
    mf, _ = _user_side_model(case)
    folded_users = mf.fold_in_users(case.data("user", True), case.n_new, case.n_passes)
    fm, sides, prob, lr, _ = _flow(12, "item")
    folded_cols = fm.fold_in_items(sides, prob.new_rows, prob.data, 1, lr=lr)
    user_prob = fc.flow_problem(12, "user")
    folded_user_cols = fm.fold_in_users(sides, user_prob.new_rows, user_prob.data, 1, lr=lr)
    calls = {"mf": (lambda **kw: mf.recommend_users(3, **kw), lambda **kw: mf.rank_audience(3, **kw),
                    lambda **kw: mf.rank_users([0], [0], **kw)),
             "fm": (lambda **kw: fm.recommend_users(sides, 3, **kw), lambda **kw: fm.rank_audience(sides, 3, **kw),
                    lambda **kw: fm.rank_users(sides, [0], [0], **kw))}
    for call in calls["mf"]:
        with pytest.raises(TypeError, match="new_items takes the FoldedRows of fold_in_items"):
            call(new_items=folded_users)           # folded users are not items
        with pytest.raises(TypeError, match="new_items takes the FoldedRows of fold_in_items"):
            call(new_items=folded_cols)            # the other model class
    with pytest.raises(TypeError, match="new_users takes the FoldedRows of fold_in_users"):  # the forward counterpart
        mf.recommend(3, new_users=folded_cols)
    for call in calls["fm"]:
        with pytest.raises(TypeError, match="new_items of an FM model takes the FoldedColumns of its fold_in_items"):
            call(new_items=folded_user_cols)
        with pytest.raises(TypeError, match="new_items of an FM model takes the FoldedColumns of its fold_in_items"):
            call(new_items=folded_users)
    with pytest.raises(TypeError, match="new_users of an FM model takes the FoldedColumns of its fold_in_users"):
        fm.recommend_users(sides, 3, new_users=folded_cols)   # new_users= given folded items stays what it is
    # another factor count
    mf13, _ = _user_side_model(_flow_case(k=13))
    items13 = _flow_case("flow-items", n_fixed=N_OLD, k=13)
    from oracle import cpu_ref
    from test_gpu_fold_in import _model
    F, fb = items13.fixed()
    _, Q, _, bi = cpu_ref.mf_init(13, 1, N_ITEMS, 13)
    rows13 = _model(N_OLD, N_ITEMS, F, Q, fb, bi).fold_in_items(items13.data("item", True), items13.n_new, 1)
    with pytest.raises(ValueError, match=r"folded rows of \(5, 13\) for a model of 12 factors"):
        mf.recommend_users(3, new_items=rows13)
    fm13, sides13, prob13, lr13, _ = _flow(13, "item")
    cols13 = fm13.fold_in_items(sides13, prob13.new_rows, prob13.data, 1, lr=lr13)
    with pytest.raises(ValueError, match=r"folded operands of \(5, 16\) for a model of 12 factors"):
        fm.recommend_users(sides, 3, new_items=cols13)
    # k, depth, ids and exclude: the forward methods' errors
    for model, lead, n_users, n_items in ((mf, (), N_OLD, N_ITEMS), (fm, (sides,), fc.FLOW_USERS, fc.FLOW_ITEMS)):
        for k in (0, 65):
            with pytest.raises(ValueError, match="outside 1..64"):
                model.recommend_users(*lead, k)
            with pytest.raises(ValueError, match="outside 1..64"):
                model.recommend(*lead, k)
        with pytest.raises(ValueError, match="depth=0"):
            model.rank_audience(*lead, 0)
        with pytest.raises(ValueError, match=f"an item id lies outside 0..{n_items - 1}"):
            model.recommend_users(*lead, 3, items=[n_items])
        with pytest.raises(ValueError, match=f"a user id lies outside 0..{n_users - 1}"):
            model.rank_users(*lead, [0], [n_users])
        with pytest.raises(ValueError, match="exclude has shape"):
            model.recommend_users(*lead, 3, exclude=sp.csr_matrix((n_items, n_users)))  # by item: the wrong way round
        with pytest.raises(ValueError, match="exclude has shape"):
            model.recommend(*lead, 3, exclude=sp.csr_matrix((n_items, n_users)))
        with pytest.raises(ValueError, match="workspace_bytes=8 is less than one block"):
            model.rank_audience(*lead, 3, workspace_bytes=8)
    with pytest.raises(TypeError, match="sides must be a recommend.Sides"):
        fm.recommend_users(None, 3)
