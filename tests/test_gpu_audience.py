"""The item -> users direction on the device through the raw ABI (include/rfm_audience.h, DESIGN.md 8
N23; needs an MI355X: ``pytest -m gpu``): rfm_pair_topk_by_item, rfm_pair_ranks_by_item and
rfm_pair_order_by_item against the FORWARD entries' bytes.  The forward logits Z[u][i] are harvested
through ``rfm_pair_topk_raw`` (64-item slices, k = 64) and the forward scores through
``rfm_pair_scores``; the by-item entries must then return the host ranking of Z transposed under the
total order (logit descending, then user index descending), every value with the forward bytes --
which an implementation that only exchanges the two tables does not give (test_audience_host.py holds
the condition on the inputs).  On top of that every result is held to the long-double oracle of
pair_tile_common at its tolerance, unwidened.  Sentinels stand behind every output."""
import numpy as np
import pytest

import audience_common as ac
import pair_tile_common as pc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rfm():
    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import features, recommend, runtime
    return pkg, features, recommend, runtime.Runtime.get()


def _assert_tile_class(n_sel, n_users, k):
    """The launches of a by-item call: rfm_pair_geometry with the counts exchanged."""
    g = pc.geometry(n_sel, n_users, k)
    full, q = pc.kpad_class(k)
    assert (g["kpad"], g["chunks"], g["tail_quarter"]) == (pc.pad4(k), full + 1, q), g
    assert (g["user_tiles"], g["item_tiles"]) == (-(-n_sel // pc.TILE), -(-n_users // pc.TILE)), g
    return g


def _forward(rfm, ops):
    """``(Zt, St)``: the forward logits and scores [n_users, n_items], transposed."""
    return ac.forward_logits(rfm, *ops).T.copy(), pc.scores(rfm, *ops).T.copy()


# --------------------------------------------------------------------------- the bitwise case
@pytest.mark.parametrize("n_items,n_users,k", ac.BITWISE_CASES)
def test_lists_are_the_ranking_of_the_forward_logits_with_their_bytes(rfm, n_items, n_users, k):
    ops = ac.operands(n_items, n_users, k)
    what = f"{n_items} items x {n_users} users k={k}"
    _assert_tile_class(n_items, n_users, k)
    og = pc.order_geometry(n_users, n_users)
    assert (og["P"], og["pages"]) == (256, 1)
    Zt, St = _forward(rfm, ops)
    assert not np.isnan(Zt).any()
    o = ac.by_item_oracle(*ops)
    pc.assert_within(Zt, o.z, o.tol_z, what + " harvested logits")
    K = 64
    users, values = ac.topk_by_item(rfm, *ops, K, raw=True)
    ac.assert_lists(users, values, Zt, K, None, None, what + " topk raw")
    ac.assert_against_oracle(users, values, o, K, None, None, what + " topk raw", raw=True)
    users, scores = ac.topk_by_item(rfm, *ops, K, raw=False)
    ac.assert_lists(users, scores, Zt, K, None, None, what + " topk", values_of=St)
    deep, dscores, n_ranked = ac.order_by_item(rfm, *ops, n_users)
    ac.assert_lists(deep, dscores, Zt, n_users, None, None, what + " order", n_ranked, values_of=St)
    ac.assert_against_oracle(deep, dscores, o, n_users, None, None, what + " order", raw=False)
    m = min(K, n_users)
    assert ac.same_bytes(deep[:, :m], users[:, :m]) and ac.same_bytes(dscores[:, :m], scores[:, :m])


# --------------------------------------------------------------------------- walks
_walk_cache = {}


def _walk_case(rfm, n_users, k, with_exclusions):
    key = (n_users, k, with_exclusions)
    if key not in _walk_cache:
        ops = ac.operands(ac.WALK_ITEMS, n_users, k)
        M = None
        if with_exclusions:
            A, LU, B, LI, c = ops
            A = np.array(A)
            A[ac.WALK_NAN_USER] = np.nan  # a user that is never ranked
            ops = (A, LU, B, LI, c)
            M = ac.walk_exclusions(n_users, ac.WALK_USERS[n_users][1])
        Zt, St = _forward(rfm, ops)
        o = ac.by_item_oracle(*ops)
        pc.assert_within(Zt, o.z, o.tol_z, f"walk {n_users} users k={k} harvested logits")
        _walk_cache[key] = (ops, o, M, Zt, St)
    return _walk_cache[key]


@pytest.mark.parametrize("with_exclusions", [False, True], ids=["plain", "exclusions"])
@pytest.mark.parametrize("k", ac.WALK_FACTORS)
@pytest.mark.parametrize("n_users", list(ac.WALK_USERS))
@pytest.mark.parametrize("n_sel", ac.WALK_SEL)
def test_workgroups_that_walk_several_user_tiles(rfm, n_sel, n_users, k, with_exclusions):
    ops, o, M, Zt, St = _walk_case(rfm, n_users, k, with_exclusions)
    g = _assert_tile_class(n_sel, n_users, k)
    assert (g["item_tiles"], g["tiles_per_split"], g["n_splits"], g["last_split_tiles"]) == ac.WALK_USERS[n_users]
    assert g["user_tiles"] == 33 and n_sel - 32 * pc.TILE in (pc.TILE, 1)
    sel = pc.walk_selection(n_sel)  # (ids below 70: here they name items)
    excl = None if M is None else pc.mask_csr(M)
    what = f"n_sel={n_sel} n_users={n_users} k={k}"
    if M is not None:
        lo = g["tiles_per_split"] * pc.TILE
        assert M[ac.WALK_EMPTY_SPLIT_ITEM, lo:2 * lo].all() and M[ac.WALK_EMPTY_SPLIT_ITEM].sum() == lo
        assert M[ac.WALK_EMPTY_ITEM].all() and np.isnan(Zt[:, ac.WALK_NAN_USER]).all()
    for K in ac.WALK_K:
        users, values = ac.topk_by_item(rfm, *ops, K, item_ids=sel, excl=excl, raw=True)
        ac.assert_lists(users, values, Zt, K, sel, M, f"{what} K={K} raw")
        ac.assert_against_oracle(users, values, o, K, sel, M, f"{what} K={K} raw", raw=True)
        users, scores = ac.topk_by_item(rfm, *ops, K, item_ids=sel, excl=excl, raw=False)
        ac.assert_lists(users, scores, Zt, K, sel, M, f"{what} K={K}", values_of=St)
        if M is not None:
            assert (users[sel == ac.WALK_EMPTY_ITEM] == -1).all() and not (users == ac.WALK_NAN_USER).any()
    tgt_indptr, tgt_users = pc.walk_targets(n_users, sel)
    ranks, rscores, cand = ac.ranks_by_item(rfm, *ops, tgt_indptr, tgt_users, item_ids=sel, excl=excl)
    want_ranks, want_cand = ac.expected_ranks(Zt, sel, tgt_indptr, tgt_users, M)
    np.testing.assert_array_equal(ranks, want_ranks)
    np.testing.assert_array_equal(cand, want_cand)
    items = np.repeat(sel, 5)
    ranked = ranks >= 0
    assert ac.same_bytes(rscores[ranked], St[items, tgt_users][ranked]) and np.isnan(rscores[~ranked]).all()
    np.testing.assert_array_equal(~ranked, np.isnan(Zt[items, tgt_users]))
    checked = 0
    for t in range(0, len(items), 7):  # the oracle's rank at the separated targets
        rank, separated = pc.oracle_rank(o, int(items[t]), int(tgt_users[t]), None if M is None else M[items[t]])
        if separated:
            assert ranks[t] == rank, (t, ranks[t], rank)
            checked += 1
    assert checked >= 0.99 * len(range(0, len(items), 7))


# --------------------------------------------------------------------------- exclusions
def test_fewer_rankable_users_than_k_and_an_item_without_any(rfm):
    n_items, n_users, k = 65, 129, 37
    ops = ac.operands(n_items, n_users, k)
    _assert_tile_class(n_items, n_users, k)
    Zt, St = _forward(rfm, ops)
    o = ac.by_item_oracle(*ops)
    M = np.zeros((n_items, n_users), dtype=bool)
    M[0] = True                        # nobody left
    M[1] = True
    M[1, [3, 64, 128]] = False         # three users left, one in each tile
    M[2, :64] = True                   # the first tile emptied
    M[64, 1::2] = True
    excl = pc.mask_csr(M)
    for K in (1, 9, 64):
        users, values = ac.topk_by_item(rfm, *ops, K, excl=excl, raw=True)
        ac.assert_lists(users, values, Zt, K, None, M, f"K={K}")
        ac.assert_against_oracle(users, values, o, K, None, M, f"K={K}", raw=True)
        assert (users[0] == -1).all() and np.isnan(values[0]).all()
        if K >= 3:
            assert sorted(users[1][users[1] >= 0].tolist()) == [3, 64, 128]
        assert (users[2][users[2] >= 0] >= 64).all()
    deep, dscores, n_ranked = ac.order_by_item(rfm, *ops, n_users + 7, excl=excl)
    ac.assert_lists(deep, dscores, Zt, n_users + 7, None, M, "order past the users", n_ranked, values_of=St)
    assert n_ranked[:3].tolist() == [0, 3, 65] and (deep[:, n_users:] == -1).all()
    # no list at all is the plain ranking
    users, values = ac.topk_by_item(rfm, *ops, 9, raw=True)
    ac.assert_lists(users, values, Zt, 9, None, None, "no list")


# --------------------------------------------------------------------------- ties
def test_ties_go_to_the_higher_user_index(rfm):
    n_items, n_users, k = 9, 130, 6
    rng = np.random.default_rng(77)
    # small integers: every product and sum is exact, and many logits are exactly equal
    A = rng.integers(-2, 3, size=(n_users, k)).astype(np.float64)
    B = rng.integers(-2, 3, size=(n_items, k)).astype(np.float64)
    LU = rng.integers(-1, 2, size=n_users).astype(np.float64)
    LI = rng.integers(-1, 2, size=n_items).astype(np.float64)
    A[100], LU[100] = A[31], LU[31]    # two identical user rows
    B[4] = 0.0                         # an item to which every user with the same LU is the same
    c = 3.0
    Zt = (c + LU[None, :] + LI[:, None]) + B @ A.T
    ops = (A, LU, B, LI, c)
    forward, St = _forward(rfm, ops)
    assert ac.same_bytes(forward, Zt), "integer operands: the device logits are exact"
    assert all(len(np.unique(row)) < n_users / 2 for row in Zt)
    for K in (1, 9, 64):
        users, values = ac.topk_by_item(rfm, *ops, K, raw=True)
        ac.assert_lists(users, values, Zt, K, None, None, f"ties K={K}")
    deep, dscores, n_ranked = ac.order_by_item(rfm, *ops, n_users)
    ac.assert_lists(deep, dscores, Zt, n_users, None, None, "ties order", n_ranked, values_of=St)
    for i, row in enumerate(deep):
        row = row.tolist()
        first, second = row.index(100), row.index(31)
        assert first < second, "two identical user rows: the higher index comes first"
        between = row[first:second + 1]  # (other users may tie with the two: all of them in descending index)
        assert len(set(Zt[i, between].tolist())) == 1 and (np.diff(between) < 0).all()
    tied = deep[4][LU[deep[4]] == 1.0]
    assert len(tied) > 10 and (np.diff(tied) < 0).all()


# --------------------------------------------------------------------------- invalid inputs
def test_selections_repeats_outside_ids_and_non_finite_rows(rfm, monkeypatch):
    monkeypatch.delenv("RFM_CHECK_IDS", raising=False)
    n_items, n_users, k = 7, 129, 37
    ops = ac.operands(n_items, n_users, k)
    A, LU, B, LI, c = ops
    rng = np.random.default_rng(130)
    sel = np.concatenate([rng.permutation(n_items), rng.integers(0, n_items, size=130 - n_items)]).astype(np.int32)
    assert _assert_tile_class(len(sel), n_users, k)["user_tiles"] == 3
    Zt, St = _forward(rfm, ops)
    K = 9
    users, values = ac.topk_by_item(rfm, *ops, K, item_ids=sel, raw=True)
    ac.assert_lists(users, values, Zt, K, sel, None, "130 selected of 7 items")
    # ids outside the table: exactly those lists are empty, every other keeps its bytes
    at = [0, 63, 64, 129]
    bad = sel.copy()
    bad[at] = [n_items, -1, 1000, np.iinfo(np.int32).max]
    got_users, got_values = ac.topk_by_item(rfm, *ops, K, item_ids=bad, raw=True)
    ac.assert_lists(got_users, got_values, Zt, K, bad, None, "ids outside the table")
    assert (got_users[at] == -1).all() and np.isnan(got_values[at]).all()
    deep, dscores, n_ranked = ac.order_by_item(rfm, *ops, n_users, item_ids=bad)
    ac.assert_lists(deep, dscores, Zt, n_users, bad, None, "ids outside the table, order", n_ranked, values_of=St)
    assert (n_ranked[at] == 0).all()
    tgt_indptr = np.arange(0, 2 * len(bad) + 1, 2)
    tgt_users = np.tile([5, 128], len(bad))
    ranks, rscores, cand = ac.ranks_by_item(rfm, *ops, tgt_indptr, tgt_users, item_ids=bad)
    want_ranks, want_cand = ac.expected_ranks(Zt, bad, tgt_indptr, tgt_users)
    np.testing.assert_array_equal(ranks, want_ranks)
    np.testing.assert_array_equal(cand, want_cand)
    assert (ranks.reshape(-1, 2)[at] == -1).all() and np.isnan(rscores.reshape(-1, 2)[at]).all() and (cand[at] == 0).all()
    # a NaN and an Inf in one row of B (an item) empty that item's lists only; in one row of A (a
    # user), that user is nobody's candidate and every other position keeps its bytes
    B2, A2 = np.array(B), np.array(A)
    B2[3, 1], B2[3, 5] = np.nan, np.inf
    got_users, got_values = ac.topk_by_item(rfm, A, LU, B2, LI, c, K, item_ids=sel, raw=True)
    assert (got_users[sel == 3] == -1).all() and np.isnan(got_values[sel == 3]).all()
    assert ac.same_bytes(got_users[sel != 3], users[sel != 3]) and ac.same_bytes(got_values[sel != 3], values[sel != 3])
    A2[70, 2], A2[70, 30] = np.nan, np.inf
    Zt2 = Zt.copy()
    Zt2[:, 70] = np.nan
    got_users, got_values = ac.topk_by_item(rfm, A2, LU, B, LI, c, 64, item_ids=sel, raw=True)
    ac.assert_lists(got_users, got_values, Zt2, 64, sel, None, "a user row with a NaN and an Inf")
    assert not (got_users == 70).any()
    deep, _, n_ranked = ac.order_by_item(rfm, A2, LU, B, LI, c, n_users, item_ids=sel)
    assert (n_ranked == n_users - 1).all() and not (deep == 70).any()


# --------------------------------------------------------------------------- ranks
@pytest.mark.parametrize("with_exclusions", [False, True], ids=["plain", "exclusions"])
@pytest.mark.parametrize("k", ac.EDGE_FACTORS)
def test_rank_of_every_pair_is_its_position_in_the_host_ranking(rfm, k, with_exclusions):
    n_items, n_users = ac.BITWISE_SHAPE
    ops = ac.operands(n_items, n_users, k)
    _assert_tile_class(n_items, n_users, k)
    Zt, St = _forward(rfm, ops)
    o = ac.by_item_oracle(*ops)
    M = None
    if with_exclusions:
        M = np.random.default_rng(k).random((n_items, n_users)) < 0.3
        M[6] = True    # an item that excludes every user
        M[7] = False
    excl = None if M is None else pc.mask_csr(M)
    tgt_indptr = np.arange(0, n_items * n_users + 1, n_users)
    tgt_users = np.tile(np.arange(n_users), n_items)
    ranks, rscores, cand = ac.ranks_by_item(rfm, *ops, tgt_indptr, tgt_users, excl=excl)
    ranks = ranks.reshape(n_items, n_users)
    want_users, _, want_n = ac.expected_lists(Zt, n_users, None, M)
    np.testing.assert_array_equal(cand, want_n)
    np.testing.assert_array_equal(cand, (~M).sum(axis=1) if M is not None else np.full(n_items, n_users))
    for i in range(n_items):
        order = want_users[i][:want_n[i]]
        np.testing.assert_array_equal(ranks[i, order], np.arange(len(order)), err_msg=f"item {i}")
    want_ranks, _ = ac.expected_ranks(Zt, np.arange(n_items), tgt_indptr, tgt_users, M)
    np.testing.assert_array_equal(ranks.reshape(-1), want_ranks)
    if M is not None:
        # a target that its item's list names is ranked against the candidates, as the forward twin
        # documents: it counts the candidates in front of it and is none of them
        i, u = 0, int(np.flatnonzero(M[0])[0])
        assert ranks[i, u] == int(((Zt[i] > Zt[i, u]) & ~M[i]).sum()) and (ranks[6] == 0).all() and cand[6] == 0
    assert ac.same_bytes(rscores.reshape(n_items, n_users), St)
    pc.assert_within(rscores.reshape(n_items, n_users), o.p, o.tol_p, f"k={k} rank scores")
    # ... and the direction agrees with itself: the rank of the r-th user of the list is r
    users, _ = ac.topk_by_item(rfm, *ops, 64, excl=excl, raw=True)
    for i in range(n_items):
        listed = users[i][users[i] >= 0]
        np.testing.assert_array_equal(ranks[i, listed], np.arange(len(listed)))
