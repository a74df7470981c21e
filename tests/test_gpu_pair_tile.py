"""The catalogue kernels of csrc/rfm_pairs.hip through the raw C ABI against the
long-double oracles of pair_tile_common.py: the side sums row by row, the pair tile at every chunk
count, tail quarter and tile edge, selections, one logit in four call families, workgroups that
walk several tiles, and every list length of the ranking kernel.  Needs an MI355X: ``pytest -m
gpu``.  Every tolerance is the derived one of pair_tile_common.py; every case asserts the class it
is there for through rfm_pair_geometry / rfm_pair_order_geometry.  Each test prints its largest
error-over-tolerance ratio; with RFM_PAIR_TILE_MARGINS=<file> the run's table of them is written
there (profiles/n21/pair_tile_margins.txt is one such run: a record, not a threshold)."""
import os

import numpy as np
import pytest

import pair_tile_common as pt
import rank_catalogue_common as rcc
import test_gpu_rank_catalogue as tgc

pytestmark = pytest.mark.gpu

MARGINS = {}  # (section, class) -> largest |d| / tol of the run, or a word for an exact comparison


def _record(section, cls, ratio):
    if isinstance(ratio, str):
        MARGINS[(section, cls)] = ratio
    else:
        MARGINS[(section, cls)] = max(MARGINS.get((section, cls), 0.0), ratio)


@pytest.fixture(scope="module")
def rfm():
    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import features, recommend, runtime
    return pkg, features, recommend, runtime.Runtime.get()


@pytest.fixture(scope="module", autouse=True)
def margins_table():
    yield
    path = os.environ.get("RFM_PAIR_TILE_MARGINS")
    if path and MARGINS:
        with open(path, "w") as f:
            f.write("largest |device - oracle| / tolerance per section and class (tolerances: tests/pair_tile_common.py)\n")
            for (section, cls), ratio in MARGINS.items():
                f.write(f"{section:<28} {cls:<44} {ratio if isinstance(ratio, str) else format(ratio, '.4f')}\n")


def _kpad_name(k):
    full, q = pt.kpad_class(k)
    return f"k={k} kpad={pt.pad4(k)} chunks={full + 1} tail quarter={q}"


def _assert_tile_class(n_sel, n_items, k):
    g = pt.geometry(n_sel, n_items, k)
    full, q = pt.kpad_class(k)
    assert (g["kpad"], g["chunks"], g["tail_quarter"]) == (pt.pad4(k), full + 1, q), g
    assert (g["user_tiles"], g["item_tiles"]) == (-(-n_sel // pt.TILE), -(-n_items // pt.TILE)), g
    return g


def _same_bytes(a, b):
    return np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes()


def _along(S, items):
    return np.take_along_axis(S, items.astype(np.int64), axis=1)


# --------------------------------------------------------------------------- side sums
@pytest.mark.parametrize("k", pt.SIDE_FACTORS)
def test_side_sums_row_by_row(rfm, k):
    X, (w, V) = pt.side_matrix(), pt.side_parameters(k)
    o = pt.side_oracle(X, w, V)
    assert pt.geometry(1, 1, k)["kpad"] == o.kpad
    worst_A = worst_L = 0.0
    for n_rows in (X.n_rows,) + pt.SIDE_ROW_CUTS:
        A, L = pt.side_sums(rfm, X, w, V, n_rows)
        assert (A[n_rows:] == pt.SENTINEL_F64).all() and (L[n_rows:] == pt.SENTINEL_F64).all()
        for r in range(n_rows):
            what = f"k={k}, {n_rows} rows, row {r} ({pt.SIDE_ROW_NAMES[r]})"
            worst_A = max(worst_A, pt.assert_within(A[r, :k], o.A[r, :k], o.tol_A[r, :k], what + " A"))
            assert _same_bytes(A[r, k:], np.zeros(o.kpad - k)), what + ": the padding is not +0.0"
            if o.length[r] == 0:
                assert _same_bytes(A[r], np.zeros(o.kpad)) and _same_bytes(L[r], np.zeros(1)[0]), what
        worst_L = max(worst_L, pt.assert_within(L[:n_rows], o.L[:n_rows], o.tol_L[:n_rows], f"k={k}, {n_rows} rows, L"))
    _record("side sums A", f"k={k} kpad={o.kpad}", worst_A)
    _record("side sums L", f"k={k} kpad={o.kpad}", worst_L)


# --------------------------------------------------------------------------- tile values
@pytest.mark.parametrize("k", pt.TILE_FACTORS)
def test_scores_at_every_chunk_count_and_tail_quarter(rfm, k):
    ops, o = pt.case(*pt.TILE_SHAPE, k)
    g = _assert_tile_class(*pt.TILE_SHAPE, k)
    assert (g["user_tiles"], g["item_tiles"]) == (2, 3)
    got = pt.scores(rfm, *ops)
    _record("tile values 65 x 129", _kpad_name(k), pt.assert_within(got, o.p, o.tol_p, _kpad_name(k)))


@pytest.mark.parametrize("k", pt.EDGE_FACTORS)
def test_scores_at_every_tile_edge(rfm, k):
    worst = 0.0
    for n_sel in pt.EDGE_SIZES:
        for n_items in pt.EDGE_SIZES:
            ops, o = pt.case(n_sel, n_items, k)
            _assert_tile_class(n_sel, n_items, k)
            worst = max(worst, pt.assert_within(pt.scores(rfm, *ops), o.p, o.tol_p, f"k={k} {n_sel} x {n_items}"))
    _record("tile edges {1..129}^2", _kpad_name(k), worst)


# --------------------------------------------------------------------------- selections
def test_selections_repeats_outside_ids_and_non_finite_rows(rfm, monkeypatch):
    monkeypatch.delenv("RFM_CHECK_IDS", raising=False)
    k, n_users, n_items = 37, 7, 129
    ops, _ = pt.case(n_users, n_items, k)
    A, LU, B, LI, c = ops
    rng = np.random.default_rng(130)
    sel = np.concatenate([rng.permutation(n_users), rng.integers(0, n_users, size=130 - n_users)]).astype(np.int32)
    assert len(sel) == 130 and pt.geometry(len(sel), n_items, k)["user_tiles"] == 3
    o = pt.pair_oracle(*ops, user_ids=sel)
    got = pt.scores(rfm, *ops, user_ids=sel)
    _record("selections", _kpad_name(k), pt.assert_within(got, o.p, o.tol_p, "130 selected of 7 users"))
    for u in range(n_users):
        mine = np.flatnonzero(sel == u)
        assert len(mine) >= 2 and all(_same_bytes(got[s], got[mine[0]]) for s in mine), u
    # ids outside the table: exactly those rows are NaN, every other element keeps its bits
    at = [0, 63, 64, 129]
    bad = sel.copy()
    bad[at] = [n_users, -1, 1000, np.iinfo(np.int32).max]
    out = pt.scores(rfm, *ops, user_ids=bad)
    keep = np.setdiff1d(np.arange(130), at)
    assert np.isnan(out[at]).all() and _same_bytes(out[keep], got[keep])
    # a NaN and an Inf in one row of A reach that user's rows only; in one row of B, that item's column only
    A2, B2 = np.array(A), np.array(B)
    A2[3, 1], A2[3, 5] = np.nan, np.inf
    out = pt.scores(rfm, A2, LU, B, LI, c, user_ids=sel)
    assert np.isnan(out[sel == 3]).all() and _same_bytes(out[sel != 3], got[sel != 3])
    B2[70, 2], B2[70, 30] = np.nan, np.inf
    out = pt.scores(rfm, A, LU, B2, LI, c, user_ids=sel)
    cols = np.arange(n_items) != 70
    assert np.isnan(out[:, 70]).all() and _same_bytes(out[:, cols], got[:, cols])


# --------------------------------------------------------------------------- one logit, four call families
@pytest.mark.parametrize("k", pt.TILE_FACTORS)
def test_one_logit_in_four_call_families(rfm, k):
    n_users, n_items = pt.TILE_SHAPE
    ops, o = pt.case(n_users, n_items, k)
    _assert_tile_class(n_users, n_items, k)
    og = pt.order_geometry(n_items, n_items)
    assert (og["P"], og["pages"]) == (256, 1)
    K = 64
    S = pt.scores(rfm, *ops)
    items, top = pt.topk(rfm, *ops, K)
    assert (items >= 0).all() and _same_bytes(top, _along(S, items)), "rfm_pair_topk's scores are not rfm_pair_scores' bytes"
    # rfm_pair_ranks of the r-th returned item is r, with the same bytes (targets ascending per user)
    perm = np.argsort(items, axis=1)
    tgt = np.take_along_axis(items, perm, axis=1)
    ranks, rscores, cand = pt.ranks(rfm, *ops, np.arange(0, n_users * K + 1, K), tgt.reshape(-1))
    np.testing.assert_array_equal(ranks.reshape(n_users, K), perm)
    assert _same_bytes(rscores.reshape(n_users, K), np.take_along_axis(top, perm, axis=1)) and (cand == n_items).all()
    # rfm_pair_order: its first 64 columns are rfm_pair_topk's bytes, the deeper ones rfm_pair_scores'
    o_items, o_scores, n_ranked = pt.order(rfm, *ops, n_items)
    assert _same_bytes(o_items[:, :K], items) and _same_bytes(o_scores[:, :K], top)
    assert (o_items >= 0).all() and _same_bytes(o_scores, _along(S, o_items)) and (n_ranked == n_items).all()
    # ... and the order is the oracle's at every separated position
    want, sep, _ = pt.oracle_lists(o, n_items)
    assert sep.mean() >= 0.99 and (o_items == want)[sep].all()
    print(_kpad_name(k), "separated positions", float(sep.mean()))
    _record("four call families", _kpad_name(k), "same bytes; the oracle's order")


# --------------------------------------------------------------------------- walks
_walk_cache = {}


def _walk_case(rfm, n_items, k, with_exclusions):
    """Operands, oracle, exclusion mask and rfm_pair_scores of the 70 users: once per case."""
    key = (n_items, k, with_exclusions)
    if key not in _walk_cache:
        ops, o = pt.case(pt.WALK_USERS, n_items, k)
        M = None
        if with_exclusions:
            A, LU, B, LI, c = ops
            B = np.array(B)
            B[pt.WALK_NAN_ITEM] = np.nan
            ops = (A, LU, B, LI, c)
            o = pt.pair_oracle(*ops)
            M = pt.walk_exclusions(n_items, pt.WALK_ITEMS[n_items][1])
        S = pt.scores(rfm, *ops)
        ratio = pt.assert_within(S, o.p, o.tol_p, f"walk {n_items} items k={k} scores of the 70 users")
        _walk_cache[key] = (ops, o, M, S, ratio)
    return _walk_cache[key]


@pytest.mark.parametrize("with_exclusions", [False, True], ids=["plain", "exclusions"])
@pytest.mark.parametrize("k", pt.WALK_FACTORS)
@pytest.mark.parametrize("n_items", list(pt.WALK_ITEMS))
@pytest.mark.parametrize("n_sel", pt.WALK_SEL)
def test_workgroups_that_walk_several_tiles(rfm, n_sel, n_items, k, with_exclusions):
    ops, o, M, S, ratio = _walk_case(rfm, n_items, k, with_exclusions)
    g = _assert_tile_class(n_sel, n_items, k)
    assert (g["item_tiles"], g["tiles_per_split"], g["n_splits"], g["last_split_tiles"]) == pt.WALK_ITEMS[n_items]
    assert g["user_tiles"] == 33 and n_sel - 32 * pt.TILE in (pt.TILE, 1)
    sel = pt.walk_selection(n_sel)
    first = np.full(pt.WALK_USERS, -1)
    first[sel[::-1]] = np.arange(n_sel)[::-1]  # the first selected position of every user
    excl = None if M is None else pt.mask_csr(M)
    cand_of = (~np.isnan(o.z) & (~M if M is not None else True)).sum(axis=1)
    if M is not None:
        lo = g["tiles_per_split"] * pt.TILE
        assert M[pt.WALK_EMPTY_SPLIT_USER, lo:2 * lo].all() and M[pt.WALK_EMPTY_SPLIT_USER].sum() == lo
        assert cand_of[pt.WALK_EMPTY_USER] == 0 and np.isnan(o.z[:, pt.WALK_NAN_ITEM]).all()
    for K in pt.WALK_K:
        items, top = pt.topk(rfm, *ops, K, user_ids=sel, excl=excl)
        want, sep, _ = pt.oracle_lists(o, K, users=sel, excluded=M)
        assert sep.mean() >= 0.99 and (items == want)[sep].all(), K
        np.testing.assert_array_equal(items < 0, want < 0)
        ok = items >= 0
        assert _same_bytes(top[ok], S[sel[:, None].repeat(K, axis=1)[ok], items[ok]]) and np.isnan(top[~ok]).all(), K
        assert _same_bytes(items, items[first[sel]]) and _same_bytes(top, top[first[sel]]), K  # repeated users
        if M is not None:
            assert not M[sel[:, None].repeat(K, axis=1)[ok], items[ok]].any() and not (items == pt.WALK_NAN_ITEM).any()
            assert (items[sel == pt.WALK_EMPTY_USER] == -1).all()
    tgt_indptr, tgt_items = pt.walk_targets(n_items, sel)
    ranks, rscores, cand = pt.ranks(rfm, *ops, tgt_indptr, tgt_items, user_ids=sel, excl=excl)
    np.testing.assert_array_equal(cand, cand_of[sel])
    users = np.repeat(sel, 5)
    known = {}
    checked = 0
    for t, (u, i) in enumerate(zip(users.tolist(), tgt_items.tolist())):
        if (u, i) not in known:
            known[(u, i)] = pt.oracle_rank(o, u, i, None if M is None else M[u])
        rank, separated = known[(u, i)]
        if separated:
            assert ranks[t] == rank, (t, u, i, ranks[t], rank)
            checked += 1
    assert checked >= 0.99 * len(users)
    ranked = ranks >= 0  # (a target on the NaN item row: rank -1, score NaN)
    assert _same_bytes(rscores[ranked], S[users, tgt_items][ranked]) and np.isnan(rscores[~ranked]).all()
    np.testing.assert_array_equal(~ranked, np.isnan(o.z[users, tgt_items]))
    assert (tgt_items[0::5] == 0).all() and (tgt_items[4::5] == n_items - 1).all()
    by_user = ranks.reshape(n_sel, 5)
    same_targets = (tgt_items.reshape(n_sel, 5) == tgt_items.reshape(n_sel, 5)[first[sel]])
    assert (by_user == by_user[first[sel]])[same_targets].all()
    _record("walks", f"n_sel={n_sel} n_items={n_items} k={k} {'exclusions' if with_exclusions else 'plain'}", ratio)


# --------------------------------------------------------------------------- list lengths
@pytest.mark.parametrize("n_items", pt.ORDER_ITEMS)
def test_every_list_length_of_the_ranking_kernel(rfm, n_items):
    seen = {}
    for pattern in pt.ORDER_PATTERNS:
        A, LU, B, LI, c, logit, M = pt.order_case(pattern, n_items)
        excl = pt.mask_csr(M)
        for depth in pt.order_depths(n_items):
            g, situations = pt.order_situations(n_items, depth, pattern)
            n_ranks = min(depth, n_items)
            assert g["P"] == min(4096, max(256, 1 << (n_ranks - 1).bit_length())) and g["pages"] == -(-n_ranks // g["P"])
            seen.setdefault(g["P"], set()).update(situations)
            got = pt.order(rfm, A, LU, B, LI, c, depth, excl=excl)
            tgc._check(got, rcc.expected_lists(logit, depth, M), f"{pattern} {n_items} items depth {depth} P {g['P']}")
            assert got[2][pt.ORDER_EXCLUDED_USER] == 0 and (got[0][pt.ORDER_EXCLUDED_USER] == -1).all()
    for P, situations in seen.items():
        _record("list lengths", f"n_items={n_items} P={P}", "exact; " + "; ".join(sorted(situations)))


def test_the_list_length_cases_reach_every_situation():
    found = {}
    for n_items in pt.ORDER_ITEMS:
        for depth in pt.order_depths(n_items):
            for pattern in pt.ORDER_PATTERNS:
                g, situations = pt.order_situations(n_items, depth, pattern)
                found.setdefault(g["P"], set()).update(situations)
    assert found == {P: set(pt.SITUATIONS) for P in pt.ORDER_LIST_LENGTHS}, found
