"""Host side of the pinning of the catalogue kernels (no GPU): the oracles of pair_tile_common.py
against plain dense statements, the floor under its tolerances, the conditions on its inputs, the
four mutations of the tile's host statement, and the two host-only geometry queries
(rfm_pair_geometry, rfm_pair_order_geometry) against every case list of test_gpu_pair_tile.py."""
import numpy as np
import pytest

import pair_tile_common as pt

LD = pt.LD

# (n_users, n_items, n_factors) of the floor and of the oracle check
FLOOR_CASES = [pt.TILE_SHAPE + (k,) for k in (1, 4, 33, 64, 128, 400)] + [(pt.WALK_USERS, 4160, k) for k in (5, 37)]


def _tile_cases():
    return [pt.TILE_SHAPE + (k,) for k in pt.TILE_FACTORS]


def _edge_cases():
    return [(ns, ni, k) for k in pt.EDGE_FACTORS for ns in pt.EDGE_SIZES for ni in pt.EDGE_SIZES]


def _walk_cases():
    return [(pt.WALK_USERS, ni, k) for ni in pt.WALK_ITEMS for k in pt.WALK_FACTORS]


# --------------------------------------------------------------------------- oracles
@pytest.mark.parametrize("shape", FLOOR_CASES, ids=str)
def test_pair_oracle_is_the_dense_statement(shape):
    ops, o = pt.case(*shape)
    dense = pt.pair_dense_ld(*ops)
    # two long-double orders of one sum: kpad + 4 roundings of 2^-64 each way
    bound = LD(2 * (o.kpad + 4)) * LD(2.0 ** -64) * o.S_z
    assert (np.abs(o.z - dense) <= bound).all()
    A, LU, B, LI, c = ops
    S = abs(c) + np.abs(LU)[:, None] + np.abs(LI)[None, :] + np.abs(A) @ np.abs(B).T
    assert np.allclose(o.S_z.astype(np.float64), S, rtol=1e-12)
    # a selection: rows by id, an id outside the table is a row of NaN
    sel = np.array([3, 0, 3, shape[0], -1, shape[0] - 1])
    sub = pt.pair_oracle(*ops, user_ids=sel)
    ok = [0, 1, 2, 5]
    assert (sub.z[ok] == o.z[sel[ok]]).all() and np.isnan(sub.z[[3, 4]]).all() and np.isnan(sub.p[[3, 4]]).all()


@pytest.mark.parametrize("k", pt.SIDE_FACTORS)
def test_side_oracle_is_the_dense_statement(k):
    X, (w, V) = pt.side_matrix(), pt.side_parameters(k)
    o = pt.side_oracle(X, w, V)
    D, D2 = np.zeros((X.n_rows, X.n_cols), dtype=LD), np.zeros((X.n_rows, X.n_cols), dtype=LD)
    rows = np.repeat(np.arange(X.n_rows), np.diff(X.indptr))
    np.add.at(D, (rows, X.indices), X.data.astype(LD))           # a column named twice: x adds up in A and lin,
    np.add.at(D2, (rows, X.indices), X.data.astype(LD) ** 2)     # x^2 in q
    Vl, wl = V.astype(LD), w.astype(LD)
    A = D @ Vl
    L = D @ wl + ((A * A).sum(axis=1) - (D2 @ (Vl * Vl)).sum(axis=1)) / 2
    eps = LD(2.0 ** -60)
    assert (np.abs(o.A[:, :k] - A) <= eps * (o.mag_A[:, :k] + 1)).all() and (o.A[:, k:] == 0).all()
    assert (np.abs(o.L - L) <= eps * (o.S_lin + o.S_cross + 1)).all()
    assert o.length.tolist() == [200, 1, 0, 7, 9, 8, 6, 12, 6] and o.kpad == pt.pad4(k)
    assert (o.tol_A[2] == 0).all() and o.tol_L[2] == 0 and o.L[2] == 0   # the empty row is exact
    # what the rows are there for
    at = lambda r: slice(X.indptr[r], X.indptr[r + 1])  # noqa: E731
    assert (X.data[at(3)] == 0).sum() == 1 and len(set(X.indices[at(4)])) == 8 and (X.data[at(5)] < 0).all()
    assert {0, X.n_cols - 1} <= set(X.indices[at(6)]) and len(set(X.indices[at(0)])) < 200


# --------------------------------------------------------------------------- the floor
@pytest.mark.parametrize("shape", FLOOR_CASES, ids=str)
def test_float64_stays_below_half_of_the_pair_tolerances(shape):
    ops, o = pt.case(*shape)
    k = shape[2]
    worst = 0.0
    for name, z in (("natural", pt.pair_float64(*ops)),
                    ("shuffled", pt.pair_float64(*ops, order=np.random.default_rng(k).permutation(k))),
                    ("tile order", pt.tile_statement(*ops) if shape[1] < 1000 else None)):
        if z is None:
            continue
        worst = max(worst, pt.assert_within(z, o.z, o.tol_z, f"{shape} float64 {name} logit", bound=0.5),
                    pt.assert_within(pt.sigmoid64(z), o.p, o.tol_p, f"{shape} float64 {name} score", bound=0.5))
    print(shape, "float64 over the bound, at most", worst)


@pytest.mark.parametrize("k", pt.SIDE_FACTORS)
def test_float64_stays_below_half_of_the_side_tolerances(k):
    X, (w, V) = pt.side_matrix(), pt.side_parameters(k)
    o = pt.side_oracle(X, w, V)
    one = o.length == 1
    assert one.sum() == 1 and (o.length[~one & (o.length > 0)] >= 6).all()
    for name, (A, L) in (("natural", pt.side_float64(X, w, V)),
                         ("shuffled", pt.side_float64(X, w, V, shuffle=np.random.default_rng(k)))):
        pt.assert_within(A[~one], o.A[~one], o.tol_A[~one], f"k={k} float64 {name} A", bound=0.5)
        pt.assert_within(A[one], o.A[one], o.tol_A[one], f"k={k} float64 {name} A of the one-entry row", bound=1.0)
        pt.assert_within(L, o.L, o.tol_L, f"k={k} float64 {name} L", bound=0.5)
        assert (A[:, k:] == 0).all() and not np.signbit(A[:, k:]).any()


@pytest.mark.parametrize("k", (1, 5, 64, 129))
def test_the_side_tolerance_catches_a_sum_that_only_one_hot_rows_hide(k):
    X, (w, V) = pt.side_matrix(), pt.side_parameters(k)
    o = pt.side_oracle(X, w, V)
    A, L = pt.side_float64(X, w, V, q_takes_x_once=True)
    ex = pt.excess(L, o.L, o.tol_L)
    ones = np.array([(X.data[X.indptr[r]:X.indptr[r + 1]] == 1.0).all() for r in range(X.n_rows)])  # (the empty row too)
    assert ones.tolist() == [name in ("empty", "binary") for name in pt.SIDE_ROW_NAMES]
    print(f"k={k} q takes x once: L off by {ex[~ones].min():.3g} tolerances at least; rows of ones at most {ex[ones].max():.3g}")
    assert (ex[~ones] > 1).all() and (ex[ones] <= 0.5).all()
    pt.assert_within(A, o.A, o.tol_A, f"k={k} A of the mutated statement (untouched)", bound=1.0)


# --------------------------------------------------------------------------- the inputs
@pytest.mark.parametrize("cases", [_tile_cases, _edge_cases, _walk_cases], ids=["tile values", "edges", "walks"])
def test_inputs_show_what_the_kernels_compute(cases):
    lo_p, hi_p, largest, share_sep, share_drop = 1.0, 0.0, 0.0, 1.0, 1.0
    for shape in cases():
        (A, LU, B, LI, c), o = pt.case(*shape)
        k = shape[2]
        lo_p, hi_p = min(lo_p, float(o.p.min())), max(hi_p, float(o.p.max()))
        largest = max(largest, float(np.abs(o.z).max()))
        sep = pt.separated_share(o)
        moved = np.abs(A[:, k - 1].astype(LD)[:, None] * B[:, k - 1].astype(LD)[None, :]) > o.tol_z
        assert sep >= 0.99 and moved.mean() >= 0.99, (shape, sep, moved.mean())
        share_sep, share_drop = min(share_sep, sep), min(share_drop, float(moved.mean()))
    print(f"scores in [{lo_p:.3g}, 1 - {1 - hi_p:.3g}], largest |z| {largest:.3g}, separated {share_sep:.4f}, "
          f"moved by the last factor {share_drop:.4f}")
    assert 1e-6 < lo_p and hi_p < 1 - 1e-6


# --------------------------------------------------------------------------- the mutations
MUTATION_FACTORS = (5, 33, 37, 64, 100, 125, 400)


@pytest.mark.parametrize("k", MUTATION_FACTORS)
def test_the_tolerance_catches_every_mutation_of_the_tile(k):
    n_users, n_items = pt.TILE_SHAPE
    ops, _ = pt.case(n_users, n_items, k)
    rng = np.random.default_rng(k)
    sel = np.concatenate([np.arange(n_users), rng.integers(0, n_users, size=n_users)])
    sel[[0, 7, 64]] = [7, 64, 0]  # the first half: three rows that are not their own position
    o = pt.pair_oracle(*ops, user_ids=sel)
    pt.assert_within(pt.tile_statement(*ops, user_ids=sel), o.z, o.tol_z, f"k={k} the statement itself", bound=0.5)
    full_chunks, q = pt.kpad_class(k)
    everything = np.ones(o.z.shape, dtype=bool)
    affected = {
        "tail_drops_last_factor": everything,
        # (a first chunk has nothing in front of it, a full tail already runs eight quarters)
        "tail_runs_eight_quarters": everything if full_chunks >= 1 and q < 8 else ~everything,
        "li_by_tile_local_item": everything & (np.arange(n_items) >= pt.TILE)[None, :],
        "user_row_is_s": everything & (sel != np.arange(len(sel)) % n_users)[:, None],
    }
    assert affected["user_row_is_s"][:n_users].any(axis=1).sum() == 3 and affected["user_row_is_s"][n_users:].any()
    for mutation in pt.MUTATIONS:
        z = pt.tile_statement(*ops, user_ids=sel, mutation=mutation)
        ex = pt.excess(z, o.z, o.tol_z)
        hit = affected[mutation]
        caught = float((ex[hit] > 1).mean()) if hit.any() else 1.0
        print(f"k={k} {mutation}: caught {caught:.4f} of {int(hit.sum())}, the others at most "
              f"{float(ex[~hit].max()) if (~hit).any() else 0.0:.3g}")
        assert caught >= 0.99, (k, mutation, caught)
        assert (ex[~hit] <= 0.5).all(), (k, mutation)


def test_the_mutation_factor_counts_reach_the_tails_they_are_for():
    # the second mutation can show behind 1 and 3 full chunks with a partly filled tail; a first
    # chunk (5) and full tails (64, 125 -> 128) are there as its no-ops
    classes = {k: pt.kpad_class(k) for k in MUTATION_FACTORS}
    assert {c for c in classes.values() if c[0] >= 1 and c[1] < 8} >= {(1, 1), (1, 2), (3, 1)}
    assert classes[5] == (0, 2) and classes[64] == (1, 8) and classes[125] == (3, 8)


# --------------------------------------------------------------------------- geometry
def test_tile_geometry_of_every_factor_count():
    classes = set()
    for k in pt.TILE_FACTORS:
        g = pt.geometry(*pt.TILE_SHAPE, k)
        full_chunks, q = pt.kpad_class(k)
        assert (g["kpad"], g["chunks"], g["tail_quarter"]) == (pt.pad4(k), full_chunks + 1, q), (k, g)
        assert (g["user_tiles"], g["item_tiles"]) == (2, 3), (k, g)
        if k in pt.KPAD_CLASSES:
            assert g["kpad"] == k
            classes.add((g["chunks"] - 1, g["tail_quarter"]))
    assert classes == {(c, q) for c in (0, 1, 3) for q in range(1, 9)}
    # the padded operands: kpad > k at 1, 2, 3 quarters; the upper bound: 32 full chunks
    assert [pt.geometry(1, 1, k)["kpad"] - k for k in (1, 2, 3, 33, 34, 35, 125)] == [3, 2, 1, 3, 2, 1, 3]
    g = pt.geometry(1, 1, 1024)
    assert (g["chunks"], g["tail_quarter"]) == (32, 8)
    # the constants that the host statement of the tile restates
    assert pt.geometry(pt.TILE, pt.TILE, pt.CHUNK)["chunks"] == 1 and pt.geometry(1, 1, pt.CHUNK + 1)["chunks"] == 2
    g = pt.geometry(pt.TILE + 1, pt.TILE, 4)
    assert (g["user_tiles"], g["item_tiles"]) == (2, 1)
    for bad in ((0, 1, 4), (1, 0, 4), (1, 1, 0), (1, 1, 1025)):
        with pytest.raises(ValueError):
            pt.geometry(*bad)


def test_tile_geometry_of_the_edges_and_the_walks():
    for ns, ni, k in _edge_cases():
        g = pt.geometry(ns, ni, k)
        assert (g["user_tiles"], g["item_tiles"]) == (-(-ns // pt.TILE), -(-ni // pt.TILE)), (ns, ni, g)
        assert g["tiles_per_split"] == 1 and g["n_splits"] == g["item_tiles"] and g["last_split_tiles"] == 1
    assert {pt.geometry(n, n, 5)["user_tiles"] for n in pt.EDGE_SIZES} == {1, 2, 3}
    for n_sel in pt.WALK_SEL:
        for ni, want in pt.WALK_ITEMS.items():
            for k in pt.WALK_FACTORS:
                g = pt.geometry(n_sel, ni, k)
                assert g["user_tiles"] == 33 and g["user_tiles"] * g["item_tiles"] > 1024
                assert (g["item_tiles"], g["tiles_per_split"], g["n_splits"], g["last_split_tiles"]) == want, (n_sel, ni, g)
                assert 1 <= g["last_split_tiles"] < g["tiles_per_split"]  # a short last split
    assert pt.WALK_SEL[0] % pt.TILE == 0 and pt.WALK_SEL[1] % pt.TILE == 1 and 2049 % pt.TILE == 1
    assert (pt.geometry(5, 37, 5)["kpad"], pt.geometry(5, 37, 37)["chunks"], pt.geometry(5, 37, 37)["tail_quarter"]) == (8, 2, 2)


def test_topk_workspace_is_the_splits_lists():
    seen = 0
    for n_sel, ni in [(ns, n) for ns in pt.WALK_SEL for n in pt.WALK_ITEMS] + [pt.TILE_SHAPE, (1, 1), (1, 129), (64, 64)]:
        for K in pt.WALK_K:
            g, ws = pt.geometry(n_sel, ni, 5), pt.topk_workspace(n_sel, ni, K)
            lists = g["n_splits"] * n_sel * K * 12
            assert ws == max(16, lists), (n_sel, ni, K, g, ws)
            seen += lists > 16
    assert seen >= 3 * 4 + 3 and pt.topk_workspace(1, 1, 1) == 16  # the floor itself is reached too


def test_order_geometry_and_the_situations_of_every_list_length():
    found = {P: set() for P in pt.ORDER_LIST_LENGTHS}
    for n_items in pt.ORDER_ITEMS:
        for depth in pt.order_depths(n_items):
            n_ranks = min(depth, n_items)
            P = min(4096, max(256, 1 << (n_ranks - 1).bit_length()))
            for pattern in pt.ORDER_PATTERNS:
                g, situations = pt.order_situations(n_items, depth, pattern)
                assert g == dict(P=P, pass_len=min(P, 1024), threshold=P - min(P, 1024), pages=-(-n_ranks // P)), \
                    (n_items, depth, g)
                found[P] |= situations
    print({P: sorted(s) for P, s in found.items()})
    for P in pt.ORDER_LIST_LENGTHS:
        assert found[P] == set(pt.SITUATIONS), (P, found[P])
    assert pt.order_geometry(8197, 8197)["pages"] == 3 and pt.order_geometry(5121, 5121)["pages"] == 2
    # the staging area takes more than one pass between flushes at 2 048 and 4 096 only
    assert [P for P in pt.ORDER_LIST_LENGTHS if pt.order_geometry(P, P)["threshold"] > 0] == [2048, 4096]
    for bad in ((0, 1), (1, 0), (1, -3)):
        with pytest.raises(ValueError):
            pt.order_geometry(*bad)
