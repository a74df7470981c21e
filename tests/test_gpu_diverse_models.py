"""recommend_diverse of both model classes on the N5 fixtures (tests/golden/recommend*.npz; DESIGN.md 8
N24): trade_off = 1 is recommend(k) byte for byte; at 0.5 and 0.3 the lists are the float64 statement
of diverse_common.py run on rank_catalogue(depth)'s own output and the normalised item rows, every
item is one of the user's candidates and none is excluded; user selections with repeats, folded-in
users, the dot product, a propensity penalty through CatalogueExposure, the errors -- and
rank_catalogue itself still returns rfm_pair_order's bytes.  Needs an MI355X: ``pytest -m gpu``.

On the code before this feature every test here fails: the methods do not exist."""
import numpy as np
import pytest
from scipy import sparse as sp

import diverse_common as dc
import pair_tile_common as pc
import rank_catalogue_common as rcc
import recommend_common as rc

pytestmark = pytest.mark.gpu

SUBSET = np.array([5, 60, 0, 5, 17, 33, 5])  # not monotone, one id three times
K = 9


@pytest.fixture(scope="module")
def rfm():
    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import features, recommend, runtime
    return pkg, features, recommend, runtime.Runtime.get()


def _models(rfm):
    """``(name, model, sides or None)`` of the fixture models: MF at both factor counts, FM on both layouts."""
    from test_gpu_recommend import _fixture_model, _mf_model
    gold = rcc.gold()
    out = [(f"mf k={k}", _mf_model(rfm[0], gold[0], k), None) for k in rc.MF_FACTORS]
    for layout, (k, alpha) in (("kuairec", (16, 0.25)), ("coat", (33, 2.0))):
        fm, sides, _, _ = _fixture_model(rfm, gold, layout, k, alpha)
        out.append((f"fm {layout} k={k}", fm, sides))
    return out


def _call(model, sides, name, *args, **kwargs):
    method = getattr(model, name)
    return method(*args, **kwargs) if sides is None else method(sides, *args, **kwargs)


def _item_rows(rfm, model, sides, metric):
    """The item table the selection takes, on the host: Q / the side sums b_i, through the device's own
    rfm_rows_normalise for the cosine (pinned bit for bit by test_gpu_neighbours.py)."""
    recommend, rt = rfm[2], rfm[3]
    ops = recommend.operands(model, sides)
    R = recommend.normalised(rt, ops.B, ops.n_factors)[0] if metric == "cosine" else ops.B
    rt.sync()
    return R.cpu().numpy()[:, :ops.n_factors], ops.n_factors


def _expected(rfm, model, sides, k, depth, lam, metric="cosine", penalty=None, **request):
    """The statement on rank_catalogue(depth)'s output -> (its four outputs, the candidates)."""
    depth = rfm[2].check_diverse(rc.N_ITEMS, k, depth)[1]
    cand = _call(model, sides, "rank_catalogue", depth, **request)
    R, kf = _item_rows(rfm, model, sides, metric)
    return dc.select_statement(cand[0], cand[1], R, kf, penalty, lam, k), cand


def _same(got, want, what):
    dc.assert_same_bits(got, want[:3], what)


def test_rank_catalogue_returns_rfm_pair_order_s_bytes(rfm):
    recommend, rt = rfm[2], rfm[3]
    g = rcc.gold()[0]
    _, model, _ = _models(rfm)[1]
    k = rc.MF_FACTORS[1]
    operands = (g[f"mf_k{k}_P"], g[f"mf_k{k}_bu"], g[f"mf_k{k}_Q"], g[f"mf_k{k}_bi"], float(g[f"mf_k{k}_b"]))
    E = sp.csr_matrix(rcc.train_mask())
    for depth, users, exclude in ((64, None, None), (rc.N_ITEMS, SUBSET, E), (300, None, E)):
        got = model.rank_catalogue(depth, users, exclude)
        want = pc.order(rfm, *operands, depth, user_ids=users, excl=None if exclude is None else pc.mask_csr(rcc.train_mask()))
        for a, b in zip(got, want):
            assert a.dtype == b.dtype and a.tobytes() == b.tobytes(), f"rank_catalogue depth={depth}"
        dev = recommend.rank_catalogue_device(*recommend.operands(model), depth, users, exclude)
        rt.sync()
        for a, b in zip(dev, got):
            assert a.is_cuda and a.cpu().numpy().tobytes() == b.tobytes(), "the device form is the same call"
    empty = recommend.rank_catalogue(*recommend.operands(model), 7, users=np.zeros(0, np.int64))
    assert [a.shape for a in empty] == [(0, 7), (0, 7), (0,)] and [a.dtype for a in empty] == [np.int32, np.float64, np.int32]


def test_trade_off_one_is_recommend(rfm):
    """Through the classes trade_off = 1 without a penalty is recommend(k) (recommend.diverse serves it
    through topk).  The selection kernel at lambda = 1 on rank_catalogue's output makes the same lists on
    every row whose first k + 1 scores are distinct doubles; saturated probabilities tie and go by item id
    (fm coat k=33, alpha = 2: 1.0 for several items of a user), which is why the class does not ask it."""
    recommend, rt = rfm[2], rfm[3]
    for name, model, sides in _models(rfm):
        want = _call(model, sides, "recommend", K)
        ops = recommend.operands(model, sides)
        cand_items, cand_scores, _ = recommend.rank_catalogue_device(*ops, 64)
        R = recommend.normalised(rt, ops.B, ops.n_factors)[0]
        picked = recommend.diversify(rt, cand_items, cand_scores, R, ops.n_factors, K, 1.0)
        distinct = (np.diff(cand_scores.cpu().numpy()[:, :K + 1], axis=1) < 0).all(axis=1)
        print(f"{name}: rows whose first {K + 1} scores are distinct: {int(distinct.sum())} of {distinct.size}")
        assert distinct.any(), name
        assert picked[0][distinct].tobytes() == want[0][distinct].tobytes(), name
        assert picked[1].tobytes() == want[1].tobytes() == picked[2].tobytes(), f"{name}: tied or not, the scores are recommend's"
        assert (picked[3][distinct] == np.arange(K)[None, :]).all(), name
        items, scores, values = _call(model, sides, "recommend_diverse", K, trade_off=1)
        assert items.tobytes() == want[0].tobytes() and scores.tobytes() == want[1].tobytes(), name
        assert values.tobytes() == scores.tobytes(), name
        E = sp.csr_matrix(rcc.train_mask())
        want = _call(model, sides, "recommend", K, SUBSET, E)
        items, scores, _ = _call(model, sides, "recommend_diverse", K, trade_off=1.0, users=SUBSET, exclude=E, metric="dot")
        assert items.tobytes() == want[0].tobytes() and scores.tobytes() == want[1].tobytes(), name


@pytest.mark.parametrize("lam", [0.5, 0.3])
def test_lists_are_the_statement_on_rank_catalogue_s_output(rfm, lam):
    M = rcc.train_mask()
    E = sp.csr_matrix(M)
    for name, model, sides in _models(rfm):
        for depth in (None, 100, 10 ** 6):
            got = _call(model, sides, "recommend_diverse", K, depth, lam, exclude=E)
            want, cand = _expected(rfm, model, sides, K, depth, lam, exclude=E)
            _same(got, want, f"{name} lambda={lam} depth={depth}")
            items = got[0]
            assert items.shape == (rc.N_USERS, K) and (items >= 0).all()
            for u in range(rc.N_USERS):
                assert np.isin(items[u], cand[0][u]).all(), f"{name}: user {u} was given an item outside its candidates"
                assert not M[u][items[u]].any(), f"{name}: user {u} was given an excluded item"
                assert len(set(items[u].tolist())) == K
        # a selection with repeats, in no order: the same user, the same list
        got = _call(model, sides, "recommend_diverse", K, None, lam, SUBSET)
        want, _ = _expected(rfm, model, sides, K, None, lam, users=SUBSET)
        _same(got, want, f"{name} lambda={lam} subset")
        assert got[0][0].tobytes() == got[0][3].tobytes() == got[0][6].tobytes()
        assert _call(model, sides, "recommend_diverse", K, None, lam, users=np.zeros(0, np.int64))[0].shape == (0, K)


def test_dot_product_metric(rfm):
    for name, model, sides in _models(rfm):
        got = _call(model, sides, "recommend_diverse", K, 64, 0.5, metric="dot")
        want, _ = _expected(rfm, model, sides, K, 64, 0.5, metric="dot")
        _same(got, want, f"{name} dot")
        cosine = _call(model, sides, "recommend_diverse", K, 64, 0.5)
        assert cosine[2].tobytes() != got[2].tobytes(), f"{name}: the metric changes nothing"


def test_propensity_penalty_lowers_the_mean_exposure(rfm):
    from relevance_factorizationmachine_amd.evaluate import CatalogueExposure
    ps = rcc.item_pscores()
    exposure = CatalogueExposure(rc.N_ITEMS, [1, 3, K], ["ME", "CatalogCoverage", "Gini"], item_pscores=ps)
    for name, model, sides in _models(rfm):
        plain = _call(model, sides, "recommend_diverse", K, 64, 0.5)
        got = _call(model, sides, "recommend_diverse", K, 64, 0.5, item_penalty=ps)
        want, _ = _expected(rfm, model, sides, K, 64, 0.5, penalty=ps)
        _same(got, want, f"{name} penalty")
        a, b = exposure.metrics(got[0]), exposure.metrics(plain[0])
        print(f"{name}: ME@k with the penalty {a['ME']}, without {b['ME']}")
        assert all(x <= y for x, y in zip(a["ME"], b["ME"])), (name, a["ME"], b["ME"])


def test_mf_folded_users(rfm):
    from test_gpu_fold_in import _flow_case, _user_side_model
    recommend, rt = rfm[2], rfm[3]
    for k in (12, 13):
        case = _flow_case(k=k)
        model, (P, Q, bu, bi) = _user_side_model(case)
        folded = model.fold_in_users(case.data("user", True), case.n_new, case.n_passes)
        n_items = Q.shape[0]
        depth = recommend.check_diverse(n_items, 3)[1]
        for users in (None, [case.n_new - 1, 0, case.n_new - 1]):
            got = model.recommend_diverse(3, trade_off=0.5, users=users, new_users=folded)
            cand = model.rank_catalogue(depth, users, new_users=folded)
            R = recommend.normalised(rt, model.Q.dev, k)[0]
            rt.sync()
            want = dc.select_statement(cand[0], cand[1], R.cpu().numpy()[:, :k], k, None, 0.5, 3)
            _same(got, want, f"mf new_users k={k}")
        own = model.recommend_diverse(3, trade_off=0.5)
        assert own[0].shape[0] == P.shape[0] and got[0].shape[0] == 3
        with pytest.raises(ValueError, match=f"a user id lies outside 0..{case.n_new - 1}"):
            model.recommend_diverse(3, users=[case.n_new], new_users=folded)
        for handle, want_bits in ((model.P, P), (model.Q, Q)):
            assert handle().tobytes() == np.asarray(want_bits).tobytes(), "the model was written"


def test_fm_folded_users(rfm):
    from test_gpu_fm_fold import _flow
    recommend, rt = rfm[2], rfm[3]
    k = 13
    model, sides, prob, lr, _ = _flow(k, "user")
    folded = model.fold_in_users(sides, prob.new_rows, prob.data, prob.n_passes, lr=lr)
    n_items = sides.n_items
    depth = recommend.check_diverse(n_items, 3)[1]
    got = model.recommend_diverse(sides, 3, trade_off=0.3, new_users=folded)
    cand = model.rank_catalogue(sides, depth, new_users=folded)
    R, kf = _item_rows(rfm, model, sides, "cosine")
    _same(got, dc.select_statement(cand[0], cand[1], R, kf, None, 0.3, 3), "fm new_users")
    assert got[0].shape == (folded.A.shape[0], 3)
    with pytest.raises(TypeError, match="new_users of an FM model takes the FoldedColumns of its fold_in_users"):
        model.recommend_diverse(sides, 3, new_users=object())


def test_errors_come_before_any_launch(rfm):
    models = _models(rfm)
    (_, mf, _), (_, fm, sides) = models[0], models[2]
    for call in (lambda **kw: mf.recommend_diverse(**kw), lambda **kw: fm.recommend_diverse(sides, **kw)):
        for k in (0, 65):
            with pytest.raises(ValueError, match="outside 1..64"):
                call(k=k)
        for lam in (-0.5, 1.5, float("nan")):
            with pytest.raises(ValueError, match=r"outside \[0, 1\]"):
                call(k=K, trade_off=lam)
        with pytest.raises(ValueError, match="k=9 picks from depth=8 candidates"):
            call(k=K, depth=8)
        with pytest.raises(ValueError, match="neither 'cosine' nor 'dot'"):
            call(k=K, metric="jaccard")
        with pytest.raises(ValueError, match="item_penalty has shape"):
            call(k=K, item_penalty=np.zeros(rc.N_ITEMS - 1))
        with pytest.raises(ValueError, match="item_penalty holds a NaN"):
            call(k=K, item_penalty=np.full(rc.N_ITEMS, np.nan))
        with pytest.raises(ValueError, match=f"a user id lies outside 0..{rc.N_USERS - 1}"):
            call(k=K, users=[rc.N_USERS])
        with pytest.raises(ValueError, match="exclude has shape"):
            call(k=K, exclude=sp.csr_matrix((rc.N_USERS, rc.N_ITEMS + 1)))
        assert call(k=K, depth=10 ** 6)[0].shape == (rc.N_USERS, K)  # (clamped to the 203 items: no error)
    with pytest.raises(TypeError, match="sides must be a recommend.Sides"):
        fm.recommend_diverse(None, K)
