"""Nearest neighbours in factor space on the device: rfm_rows_normalise bit for
bit against the NumPy statement of its order, rfm_pair_topk_raw against rfm_pair_topk and the
long-double oracle, recommend.neighbours against the oracle's lists at every separated position
and its values at the derived tolerance, exact ties, determinism across splits, and the four model
methods with fold-in.  Needs an MI355X: ``pytest -m gpu``.  Oracle, statement, tolerances and the
checkers: neighbours_common.py; test_neighbours_host.py shows that the checkers catch six mutations.

The model methods compare vectors the device sums itself (FM: b_i = sum_j xi_j V[j,:]).  A side
sum of L entries is off by at most (L + 1) u a_f per factor, a_f = sum_j |x_j V[j,f]| (pair_tile_
common: tol_A, and one rounding of the oracle's own float64 copy), so a row by d = (L + 1) u ||a||_2
in norm.  A unit vector moves by at most 2 d / ||b||, hence a cosine by at most 2 (d_i / ||b_i|| +
d_j / ||b_j||); a dot product by d_i ||b_j|| + d_j ||b_i|| (second order: times 1 + 2^-40).  That
is added to the tolerance of neighbours_common.oracle, and the separation of the oracle's order
is taken with the widened tolerance.

rfm_pair_topk's scores are sigmoid_clipped of rfm_pair_topk_raw's values, byte for byte.  The
sigmoid that shows it is the DEVICE's (rfm_pair_scores on operands that make the logit the value
itself): NumPy's exp and the device's are two correctly working exps that round some arguments
differently, so pair_tile_common.sigmoid64 on the host cannot give the device's bytes -- measured
on an MI355X at TILE_SHAPE, 1 to 7 of 621 elements (K = 9) and 77 to 83 of 4 416 (K = 64) differ,
none by more than 2.2e-16; K = 1 happened to agree.  The host's sigmoid64 is held to the 8 u p
that pair_tile_common derives for exp, add and divide.

On the code before this feature every test here fails: the symbols and the methods do not exist."""
import numpy as np
import pytest
from scipy import sparse as sp

import neighbours_common as nc
import pair_tile_common as pc
import recommend_common as rc
from conftest import load_golden
from fold_common import _bits, _n_cu
from neighbours_common import LD, U, pad4

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rfm():
    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import features, recommend, runtime
    return pkg, features, recommend, runtime.Runtime.get()


@pytest.fixture(scope="module")
def gold():
    return load_golden("recommend"), {layout: load_golden(f"recommend_fm_{layout}") for layout in rc.LAYOUTS}


def _same_bits(got, want, what):
    """Equal bytes, except that a NaN may be any NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    nan = np.isnan(want)
    assert (np.isnan(got) == nan).all(), f"{what}: NaN where a number belongs, or the reverse"
    differ = (_bits(got) != _bits(want)) & ~nan
    assert not differ.any(), (f"{what}: {int(differ.sum())} of {differ.size} elements differ; first at "
                              f"{tuple(np.argwhere(differ)[0])}: got {got[differ][0]!r}, want {want[differ][0]!r}")


# --------------------------------------------------------------------------
# rfm_rows_normalise, bit for bit
# --------------------------------------------------------------------------
@pytest.mark.parametrize("stride", ["k", "kpad"])
@pytest.mark.parametrize("k", nc.NORMALISE_FACTORS)
def test_rows_normalise_bit_for_bit(rfm, k, stride):
    kpad = pad4(k)
    M = np.vstack([nc.special_rows(k), nc.rows(257, k)])
    want_out, want_norm = nc.normalise_statement(M, k)
    nc.assert_normalised(want_out, want_norm, M, k, "the statement itself")
    for n_rows in nc.NORMALISE_ROWS + (M.shape[0],):
        out, norm = nc.normalise(rfm, M, k, n_rows, k if stride == "k" else kpad)
        what = f"k={k} ld={stride} rows={n_rows}"
        _same_bits(out[:n_rows], want_out[:n_rows], f"{what} out")
        _same_bits(norm[:n_rows], want_norm[:n_rows], f"{what} norm")
        pad = out[:n_rows, k:]
        assert not pad.any() and not np.signbit(pad).any(), f"{what}: the padding is not +0.0"
    special = dict(zip(nc.SPECIAL_ROWS, out))
    for name in ("all zero", "a NaN", "an Inf", "1e200", "1e-200"):
        assert np.isnan(special[name][:k]).all() and not special[name][k:].any(), name
    assert special["a single non-zero"][k - 1] == -1.0


def test_rows_normalise_past_one_pass_of_the_capped_grid(rfm):
    k = 5
    n = _n_cu(rfm[3]) * 8 * 4 + 5  # 8 workgroups of 4 rows per CU, then the stride
    M = nc.rows(n, k)
    want_out, want_norm = nc.normalise_statement(M, k)
    for ld in (k, pad4(k)):
        out, norm = nc.normalise(rfm, M, k, n, ld)
        _same_bits(out, want_out, f"{n} rows ld={ld} out")
        _same_bits(norm, want_norm, f"{n} rows ld={ld} norm")


def test_rows_normalise_rejects_bad_arguments(rfm):
    import torch
    _, _, recommend, rt = rfm
    M = rt.upload(np.ones((3, 5)))
    out, norm = rt.empty((3, 8), torch.float64), rt.empty((3,), torch.float64)
    call = lambda *a: rt.lib.rfm_rows_normalise(rt.ctx, *a)  # noqa: E731
    assert call(M.data_ptr(), 3, 5, 5, out.data_ptr(), norm.data_ptr()) == 0
    assert call(M.data_ptr(), 3, 5, 4, out.data_ptr(), norm.data_ptr()) == 1       # ld_in < n_factors
    assert call(M.data_ptr(), 3, 0, 5, out.data_ptr(), norm.data_ptr()) == 1
    assert call(M.data_ptr(), 3, 5, 5, M.data_ptr(), norm.data_ptr()) == 1         # in place
    assert call(None, 3, 5, 5, out.data_ptr(), norm.data_ptr()) == 1
    assert call(M.data_ptr(), 0, 5, 5, out.data_ptr(), norm.data_ptr()) == 0       # no rows: no launch
    with pytest.raises(ValueError, match="for 5 factors"):
        recommend.normalised(rt, rt.upload(np.ones((3, 6))), 5)
    rt.sync()


# --------------------------------------------------------------------------
# rfm_pair_topk_raw against rfm_pair_topk and the pair oracle
# --------------------------------------------------------------------------
RAW_NAN_ITEM, RAW_NAN_USER, RAW_SHORT_USER = 100, 7, 5


def _device_sigmoid(rfm, values):
    """sigmoid_clipped of every value by the device function itself: rfm_pair_scores of a catalogue of
    one item with A = B = 0, LI = 0, c = 0 and LU = the values, whose logit ((0 + v) + 0) + 0 is v."""
    v = np.asarray(values, dtype=np.float64).reshape(-1)
    got = pc.scores(rfm, np.zeros((v.size, 1)), v, np.zeros((1, 1)), np.zeros(1), 0.0)
    return got.reshape(np.asarray(values).shape)


def _raw_case(kf, lists):
    n_users, n_items = pc.TILE_SHAPE
    A, LU, B, LI, c = (np.array(a) for a in pc.operands(n_users, n_items, kf))
    B[RAW_NAN_ITEM] = np.nan
    A[RAW_NAN_USER] = np.nan  # a user without candidates
    M = None
    if lists:
        M = np.random.default_rng(kf).random((n_users, n_items)) < 0.1
        M[RAW_SHORT_USER] = True
        M[RAW_SHORT_USER, [0, 64, 128]] = False  # three candidates, one per item tile
    return (A, LU, B, LI, float(c)), M


@pytest.mark.parametrize("lists", [False, True])
@pytest.mark.parametrize("K", nc.NEIGHBOUR_K)
@pytest.mark.parametrize("kf", nc.RAW_FACTORS)
def test_topk_raw_items_are_topk_s_and_values_are_the_logits(rfm, kf, K, lists):
    ops, M = _raw_case(kf, lists)
    sel = np.concatenate([np.arange(pc.TILE_SHAPE[0]), [RAW_SHORT_USER, 64, 0, RAW_NAN_USER]]).astype(np.int32)
    excl = None if M is None else pc.mask_csr(M)
    items, scores = pc.topk(rfm, *ops, K, user_ids=sel, excl=excl)
    raw_items, values = nc.topk_raw(rfm, *ops, K, user_ids=sel, excl=excl)
    assert raw_items.tobytes() == items.tobytes(), "the two entries rank differently"
    o = pc.pair_oracle(*ops)
    nc.assert_lists(raw_items, values, o, K, sel, M, f"kf={kf} K={K} lists={lists}")
    assert (raw_items != RAW_NAN_ITEM).all() and (raw_items[sel == RAW_NAN_USER] == -1).all()
    if lists:
        short = raw_items[sel == RAW_SHORT_USER]
        assert ((short >= 0).sum(axis=1) == min(K, 3)).all()
    assert (np.isnan(values) == (raw_items < 0)).all() and (np.isnan(scores) == (items < 0)).all()
    # the scores are sigmoid_clipped of these very values: the device's own, bit for bit (module docstring)
    _same_bits(_device_sigmoid(rfm, values), scores, "sigmoid_clipped(values) against rfm_pair_topk's scores")
    # and the host's sigmoid64 within the 8 u p that pair_tile_common's score bound allows exp, add and divide
    host = pc.sigmoid64(values)
    off = (_bits(host) != _bits(scores)) & ~np.isnan(scores)
    print(f"sigmoid64(values) against the scores: {int(off.sum())} of {off.size} differ, largest difference "
          f"{np.nanmax(np.abs(host - scores), initial=0.0):.3g}")
    assert np.all(np.abs(host - scores)[~np.isnan(scores)] <= 8 * U * scores[~np.isnan(scores)])


# --------------------------------------------------------------------------
# neighbours through the raw ABI
# --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", nc.METRICS)
@pytest.mark.parametrize("k", nc.NEIGHBOUR_FACTORS)
@pytest.mark.parametrize("n", nc.NEIGHBOUR_ROWS)
def test_neighbours_against_the_oracle(rfm, n, k, metric):
    _, _, recommend, rt = rfm
    R = nc.rows(n, k)
    o, mask = nc.oracle(R, metric), nc.self_mask(n)
    dR = rt.upload(np.array(R))
    for K in nc.NEIGHBOUR_K:
        for sel in (None, nc.selection(n)):
            what = f"n={n} k={k} {metric} K={K} sel={'all' if sel is None else 'some'}"
            ids, values = recommend.neighbours(rt, dR, k, K, ids=sel, metric=metric)
            nc.assert_lists(ids, values, o, K, sel, mask, what)
            q = np.arange(n) if sel is None else sel
            assert (ids != q[:, None]).all(), f"{what}: a query is its own neighbour"
            ids, values = recommend.neighbours(rt, dR, k, K, ids=sel, metric=metric, include_self=True)
            nc.assert_lists(ids, values, o, K, sel, None, f"{what} include_self")
            if metric == "cosine":
                assert (ids[:, 0] == q).all(), f"{what}: self is not the first neighbour"
                assert np.all(np.abs(values[:, 0].astype(LD) - 1) <= o.tol_z[q, q])


def test_neighbours_among_rows_of_another_table(rfm):
    _, _, recommend, rt = rfm
    n, k = 129, 37
    R, Q = nc.rows(n, k), nc.rows(11, k, seed=1)
    dR, dQ = rt.upload(np.array(R)), rt.upload(np.array(Q))
    M = np.random.default_rng(5).random((11, n)) < 0.2
    for metric in nc.METRICS:
        o = nc.oracle(R, metric, Q)
        sel = np.array([10, 0, 3, 3])
        ids, values = recommend.neighbours(rt, dR, k, 9, ids=sel, metric=metric, queries=dQ)
        nc.assert_lists(ids, values, o, 9, sel, None, f"queries {metric}")
        ids, values = recommend.neighbours(rt, dR, k, 9, metric=metric, queries=dQ, exclude=sp.csr_matrix(M))
        nc.assert_lists(ids, values, o, 9, None, M, f"queries {metric} exclude")
    # the table as its own query table: rows of another table have no self to exclude
    ids, values = recommend.neighbours(rt, dR, k, 3, queries=dR)
    assert (ids[:, 0] == np.arange(n)).all()


# --------------------------------------------------------------------------
# exact ties
# --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", nc.METRICS)
def test_planted_rows_rank_by_id_descending_with_equal_bits(rfm, metric):
    _, _, recommend, rt = rfm
    n, k, K = 129, 37, 64
    R = np.array(nc.rows(n, k))
    R[70] = R[10]                 # twice, in two item tiles
    R[128] = R[40] = R[30]        # three times, the last in the one-wide edge tile
    ids, values = recommend.neighbours(rt, rt.upload(R), k, K, metric=metric)
    seen = 0
    for group in ((70, 10), (128, 40, 30)):
        for q in range(n):
            at = [int(np.flatnonzero(ids[q] == g)[0]) if (ids[q] == g).any() else -1 for g in group]
            if q in group or min(at) < 0:
                continue
            seen += 1
            assert at == list(range(at[0], at[0] + len(group))), (metric, q, group, at)
            assert len({values[q, a].tobytes() for a in at}) == 1, (metric, q, group, values[q, at])
    assert seen > n // 2
    if metric == "cosine":  # a planted row's twins come first, at cosine 1 within tolerance
        assert ids[10, 0] == 70 and ids[70, 0] == 10 and ids[30, :2].tolist() == [128, 40]
        assert abs(values[10, 0] - 1) < 64 * U


def test_one_factor_every_cosine_is_exactly_plus_or_minus_one(rfm):
    _, _, recommend, rt = rfm
    n = 129
    R = nc.rows(n, 1)
    for K in (9, 64):
        ids, values = recommend.neighbours(rt, rt.upload(np.array(R)), 1, K)
        for q in range(n):
            others = np.arange(n)[::-1]
            others = others[others != q]
            same = np.sign(R[others, 0]) == np.sign(R[q, 0])
            want = np.concatenate([others[same], others[~same]])[:K]
            assert ids[q].tolist() == want.tolist(), (K, q)
            assert values[q].tolist() == np.where(np.sign(R[want, 0]) == np.sign(R[q, 0]), 1.0, -1.0).tolist()


# --------------------------------------------------------------------------
# determinism
# --------------------------------------------------------------------------
@pytest.mark.parametrize("metric", nc.METRICS)
def test_same_bytes_twice_and_across_splits(rfm, metric, monkeypatch):
    """Two calls give the same bytes; a catalogue of 64 rows (one item tile: one split) and the same
    rows followed by 129 rows that are never ranked (NaN rows; four tiles: several splits) give the
    same bytes too, with the workspace held at the larger of the two sizes."""
    _, _, recommend, rt = rfm
    k, K = 37, 9
    R = nc.rows(64, k)
    grown = np.vstack([R, np.full((129, k), np.nan)])
    sel = np.array([63, 0, 5, 5, 31])
    assert pc.geometry(len(sel), 64, k)["n_splits"] == 1 and pc.geometry(len(sel), 193, k)["n_splits"] > 1
    size = recommend.topk_workspace_bytes(len(sel), 193, K)
    assert size > recommend.topk_workspace_bytes(len(sel), 64, K)
    monkeypatch.setattr(recommend, "topk_workspace_bytes", lambda *a: size)
    first = recommend.neighbours(rt, rt.upload(np.array(R)), k, K, ids=sel, metric=metric)
    again = recommend.neighbours(rt, rt.upload(np.array(R)), k, K, ids=sel, metric=metric)
    split = recommend.neighbours(rt, rt.upload(grown), k, K, ids=sel, metric=metric)
    for a, b, c in zip(first, again, split):
        assert a.tobytes() == b.tobytes(), "two calls differ"
        assert a.tobytes() == c.tobytes(), "the result depends on the split"
    assert (first[0] >= 0).all()


# --------------------------------------------------------------------------
# the Python surface
# --------------------------------------------------------------------------
SUBSET = np.array([5, 60, 0, 5, 17, 33, 5])  # not monotone, one id three times
EMPTY_ITEM = 17


def _widened(o, metric, q_err, q_norm, c_err, c_norm):
    """The oracle's tolerance plus what the vectors' own errors add (module docstring)."""
    q_err, q_norm, c_err, c_norm = (np.asarray(a).astype(LD) for a in (q_err, q_norm, c_err, c_norm))
    with np.errstate(all="ignore"):
        if metric == "cosine":
            more = 2 * (np.where(q_norm > 0, q_err / q_norm, 0)[:, None] + np.where(c_norm > 0, c_err / c_norm, 0)[None, :])
        else:
            more = q_err[:, None] * c_norm[None, :] + c_err[None, :] * q_norm[:, None]
    o.tol_z = o.tol_z + more * LD(nc.SECOND_ORDER)
    return o


def _side_vectors(X, V):
    """``(b float64 [n, k], error bound of a row in norm [n], norm [n])`` of a side matrix, from long double."""
    X = sp.csr_matrix(X)
    D, Vl = np.asarray(X.todense()).astype(LD), np.asarray(V).astype(LD)
    b, a = D @ Vl, np.abs(D) @ np.abs(Vl)
    err = (np.diff(X.indptr) + 1).astype(LD) * LD(U) * np.sqrt((a * a).sum(axis=1))
    return b.astype(np.float64), err, np.sqrt((b * b).sum(axis=1))


def _zeros(n):
    return np.zeros(n)


@pytest.mark.parametrize("k", rc.MF_FACTORS)
def test_mf_similar_items_and_users(rfm, gold, k):
    from test_gpu_recommend import _mf_model
    g = gold[0]
    model = _mf_model(rfm[0], g, k)
    P, Q = g[f"mf_k{k}_P"], g[f"mf_k{k}_Q"]
    for side, table, call in (("items", Q, model.similar_items), ("users", P, model.similar_users)):
        n = table.shape[0]
        for metric in nc.METRICS:
            o, mask = nc.oracle(table, metric), nc.self_mask(n)
            ids, values = call(9, metric=metric)
            nc.assert_lists(ids, values, o, 9, None, mask, f"mf k={k} {side} {metric}")
        M = mask | (np.random.default_rng(k).random((n, n)) < 0.3)
        ids, values = call(64, **{side: SUBSET}, exclude=sp.csr_matrix(M & ~mask))
        nc.assert_lists(ids, values, nc.oracle(table, "cosine"), 64, SUBSET, M, f"mf k={k} {side} subset exclude")
        ids, values = call(3, **{side: SUBSET}, include_self=True)
        assert (ids[:, 0] == SUBSET).all()
    for handle, want in ((model.P, P), (model.Q, Q)):
        assert _bits(handle()).tobytes() == _bits(want).tobytes()


@pytest.mark.parametrize("layout", rc.LAYOUTS)
@pytest.mark.parametrize("k,alpha", [(16, 0.25), (400, 2.0)])
def test_fm_similar_items_and_users(rfm, gold, layout, k, alpha):
    from test_gpu_recommend import _fm_model
    pkg, _, recommend, rt = rfm
    g, gls = gold
    w0, w, V = rc.fm_parameters(g, gls[layout], layout, k, alpha)
    XU, XI = rc.side_matrices(layout, g["user_table"], g["item_table"], g["context"])
    XI = XI.tolil()
    XI[EMPTY_ITEM] = 0  # an item without entries: no direction
    XI = XI.tocsr()
    XI.eliminate_zeros()
    assert XI.indptr[EMPTY_ITEM] == XI.indptr[EMPTY_ITEM + 1]
    sides = recommend.Sides(XU, XI)
    model = _fm_model(pkg, sides.n_features, k, alpha, w0, w, V)
    for side, X, call in (("items", XI, model.similar_items), ("users", XU, model.similar_users)):
        b, err, norm = _side_vectors(X, V)
        n = b.shape[0]
        mask = nc.self_mask(n)
        for metric in nc.METRICS:
            o = _widened(nc.oracle(b, metric), metric, err, norm, err, norm)
            if side == "items" or metric == "cosine":
                share = pc.separated_share(o, mask)
                print(f"fm {layout} k={k} {side} {metric}: separated share {share:.3f}")
            ids, values = call(sides, 9, metric=metric)
            nc.assert_lists(ids, values, o, 9, None, mask, f"fm {layout} k={k} {side} {metric}")
            if side == "items" and metric == "cosine":
                assert (ids != EMPTY_ITEM).all(), "an item without entries is somebody's neighbour"
                assert (ids[EMPTY_ITEM] == -1).all() and np.isnan(values[EMPTY_ITEM]).all()
                assert (ids[np.arange(n) != EMPTY_ITEM] >= 0).all()
        o = _widened(nc.oracle(b, "cosine"), "cosine", err, norm, err, norm)
        M = mask | (np.random.default_rng(k).random((n, n)) < 0.3)
        ids, values = call(sides, 64, **{side: SUBSET}, exclude=sp.csr_matrix(M & ~mask))
        nc.assert_lists(ids, values, o, 64, SUBSET, M, f"fm {layout} k={k} {side} subset exclude")
    for handle, want in ((model.V, V), (model.w, w)):
        assert _bits(handle()).tobytes() == _bits(np.asarray(want, dtype=np.float64)).tobytes()


def test_mf_folded_rows_are_the_queries(rfm):
    from test_gpu_fold_in import N_ITEMS, N_OLD, _flow_case, _model, _user_side_model
    from oracle import cpu_ref
    for k in (12, 13):
        case = _flow_case(k=k)
        model, (P, Q, bu, bi) = _user_side_model(case)
        folded = model.fold_in_users(case.data("user", True), case.n_new, case.n_passes)
        rows = folded.numpy()[0]
        for metric in nc.METRICS:
            ids, values = model.similar_users(3, metric=metric, new_users=folded)
            nc.assert_lists(ids, values, nc.oracle(P, metric, rows), 3, None, None, f"mf new_users k={k} {metric}")
        sel = np.array([4, 0, 4])
        ids, values = model.similar_users(9, users=sel, new_users=folded)
        assert ids.shape == (3, 9) and ids[0].tobytes() == ids[2].tobytes() and (ids[:, :N_OLD] >= 0).all()
        # a user without examples keeps its zero row: no direction, an empty list
        idle = int(np.flatnonzero(case.lengths == 0)[0])
        assert not rows[idle].any() and (model.similar_users(3, new_users=folded)[0][idle] == -1).all()
        for handle, want in ((model.P, P), (model.Q, Q), (model.b_u, bu), (model.b_i, bi)):
            assert _bits(handle()).tobytes() == _bits(want).tobytes(), "the model was written"
        # the item side: the model with the sides exchanged
        items_case = _flow_case("flow-items", n_fixed=N_OLD, k=k)
        F, fb = items_case.fixed()
        _, Qi, _, bii = cpu_ref.mf_init(13, 1, N_ITEMS, k)
        mirror = _model(N_OLD, N_ITEMS, F, Qi, fb, bii)
        new_items = mirror.fold_in_items(items_case.data("item", True), items_case.n_new, items_case.n_passes)
        ids, values = mirror.similar_items(5, new_items=new_items)
        nc.assert_lists(ids, values, nc.oracle(Qi, "cosine", new_items.numpy()[0]), 5, None, None, f"mf new_items k={k}")
        assert _bits(mirror.Q()).tobytes() == _bits(Qi).tobytes()
        with pytest.raises(TypeError, match="new_users takes the FoldedRows of fold_in_users"):
            mirror.similar_users(3, new_users=new_items)
        with pytest.raises(TypeError, match="new_items takes the FoldedRows of fold_in_items"):
            model.similar_items(3, new_items=folded)
        with pytest.raises(ValueError, match="include_self"):
            model.similar_users(3, new_users=folded, include_self=True)
        with pytest.raises(ValueError, match="a user id lies outside 0..4"):
            model.similar_users(3, users=[5], new_users=folded)
    other = _user_side_model(_flow_case(k=12))[0]
    with pytest.raises(ValueError, match=r"folded rows of \(5, 13\) for a model of 12 factors"):
        other.similar_users(3, new_users=folded)


@pytest.mark.parametrize("side", ["user", "item"])
def test_fm_folded_columns_are_the_queries(rfm, side):
    from test_gpu_fm_fold import _flow
    for k in (12, 13):
        model, sides, prob, lr, (w0, w, V) = _flow(k, side)
        fold = model.fold_in_users if side == "user" else model.fold_in_items
        call = model.similar_users if side == "user" else model.similar_items
        folded = fold(sides, prob.new_rows, prob.data, prob.n_passes, lr=lr)
        model._rt.sync()
        A = folded.A.cpu().numpy()
        assert not A[:, k:].any()
        b, err, norm = _side_vectors(prob.XU if side == "user" else prob.XI, V)
        n_new = A.shape[0]
        for metric in nc.METRICS:
            o = _widened(nc.oracle(b, metric, A[:, :k]), metric, _zeros(n_new), np.linalg.norm(A[:, :k], axis=1), err, norm)
            ids, values = call(sides, 5, metric=metric, **{f"new_{side}s": folded})
            nc.assert_lists(ids, values, o, 5, None, None, f"fm new_{side}s k={k} {metric}")
        ids, _ = call(sides, 3, **{f"{side}s": [n_new - 1, 0, n_new - 1], f"new_{side}s": folded})
        assert ids.shape == (3, 3) and ids[0].tobytes() == ids[2].tobytes()
        for handle, want in ((model.V, V), (model.w, w), (model.w0, w0)):
            assert _bits(handle()).tobytes() == _bits(np.asarray(want, dtype=np.float64).reshape(handle().shape)).tobytes()
        wrong = model.similar_items if side == "user" else model.similar_users
        other = "item" if side == "user" else "user"
        with pytest.raises(TypeError, match=f"new_{other}s of an FM model takes the FoldedColumns of its fold_in_{other}s"):
            wrong(sides, 3, **{f"new_{other}s": folded})
        with pytest.raises(ValueError, match="include_self"):
            call(sides, 3, include_self=True, **{f"new_{side}s": folded})
    # (folded, call: the 13-factor model's) another factor count, and the other model class's folded rows
    model12, sides12 = _flow(12, side)[:2]
    call12 = model12.similar_users if side == "user" else model12.similar_items
    with pytest.raises(ValueError, match=r"folded operands of \(\d+, 16\) for a model of 12 factors"):
        call12(sides12, 3, **{f"new_{side}s": folded})
    mf_rows = type("FoldedRows", (), {"side": side, "rows": np.zeros((2, 12)), "bias": np.zeros(2)})()
    with pytest.raises(TypeError, match=f"new_{side}s of an FM model takes the FoldedColumns of its fold_in_{side}s"):
        call12(sides12, 3, **{f"new_{side}s": mf_rows})


def test_model_methods_refuse_bad_arguments(rfm, gold):
    from test_gpu_recommend import _fixture_model, _mf_model
    fm, sides, _, _ = _fixture_model(rfm, gold, "coat", 16, 0.25)
    mf = _mf_model(rfm[0], gold[0], 24)
    for call in (lambda **kw: mf.similar_items(**kw), lambda **kw: fm.similar_items(sides, **kw),
                 lambda **kw: mf.similar_users(**kw), lambda **kw: fm.similar_users(sides, **kw)):
        for k in (0, 65):
            with pytest.raises(ValueError, match="outside 1..64"):
                call(k=k)
        with pytest.raises(ValueError, match="neither 'cosine' nor 'dot'"):
            call(k=3, metric="jaccard")
    with pytest.raises(ValueError, match=f"an item id lies outside 0..{rc.N_ITEMS - 1}"):
        mf.similar_items(3, items=[rc.N_ITEMS])
    with pytest.raises(ValueError, match=f"a user id lies outside 0..{rc.N_USERS - 1}"):
        fm.similar_users(sides, 3, users=[-1])
    with pytest.raises(ValueError, match="exclude has shape"):
        mf.similar_items(3, exclude=sp.csr_matrix((rc.N_ITEMS, rc.N_USERS)))
    with pytest.raises(TypeError, match="sides must be a recommend.Sides"):
        fm.similar_items(None, 3)
