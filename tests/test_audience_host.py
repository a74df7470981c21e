"""Host half of the tests of the item -> users direction (no GPU): the float64
statement of the by-item tile against the transpose of the forward statement, three mutations each
caught on the affected logits alone, the condition on the inputs that lets the bitwise GPU case tell
the by-item form from a plain exchange of the tables, the host transposition of ``exclude`` against
scipy, the header's three prototypes against the ctypes table, and the geometry of every GPU case
list."""
import os
import re
import types

import numpy as np
import pytest
from scipy import sparse as sp

import audience_common as ac
import pair_tile_common as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# the statement is held on the operands of the bitwise GPU case: every edge shape at the two edge
# factor counts, the chunk classes at the bitwise shape
STATEMENT_CASES = ac.BITWISE_CASES


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


@pytest.mark.parametrize("k", ac.EDGE_FACTORS + ac.BITWISE_FACTORS)
def test_statement_is_the_transpose_of_the_forward_statement_in_every_byte(k):
    shapes = [(ni, nu) for ni in ac.EDGE_SIZES for nu in ac.EDGE_SIZES] if k in ac.EDGE_FACTORS else [ac.BITWISE_SHAPE]
    for n_items, n_users in shapes:
        assert (n_items, n_users, k) in STATEMENT_CASES
        ops = ac.operands(n_items, n_users, k)
        forward = pc.tile_statement(*ops)
        assert forward.shape == (n_users, n_items)
        assert ac.same_bytes(ac.by_item_statement(*ops), forward.T), (n_items, n_users, k)
    # a selection of items with repeats goes through the rows of the tile
    ops = ac.operands(*ac.BITWISE_SHAPE, k)
    sel = np.array([64, 0, 64, 3, 17, 64])
    assert ac.same_bytes(ac.by_item_statement(*ops, item_ids=sel), pc.tile_statement(*ops).T[sel])


@pytest.mark.parametrize("k", ac.EDGE_FACTORS + ac.BITWISE_FACTORS)
def test_exchanged_sum_order_changes_one_logit_in_ten_on_the_bitwise_case(k):
    """A condition on the inputs, not a measurement: otherwise rfm_pair_topk_by_item could be a forward
    call with the tables exchanged and the bitwise GPU case would not notice.  One logit in ten is
    held for the operands of a factor count as a whole; a single shape of 63 logits or more must hold
    at least one changed logit, so that it can tell by itself (a share over 63 draws scatters too
    widely to be held to a tenth, and the 1 x 1 shape holds one logit: its share is 0 or 1)."""
    changed = total = 0
    for n_items, n_users, kf in ac.BITWISE_CASES:
        if kf != k:
            continue
        share = ac.changed_share(*ac.operands(n_items, n_users, k))
        print(f"{n_items} items x {n_users} users, k={k}: the exchanged order changes {share:.3f} of the logits")
        if n_items * n_users >= 63:
            assert share > 0, (n_items, n_users, k)
        changed, total = changed + share * n_items * n_users, total + n_items * n_users
    assert total and changed / total >= ac.MIN_CHANGED_SHARE


def test_mutation_side_terms_in_the_exchanged_order():
    n_items, n_users, k = 130, 70, 5
    A, LU, B, LI, c = (np.array(a) for a in ac.operands(n_items, n_users, k))
    LU[7] = 0.0   # a user without a side term: c + LI is then the whole sum either way...
    LI[11] = 0.0  # ... and so is c + LU for an item without one
    Zt = ac.by_item_statement(A, LU, B, LI, c)
    mutated = ac.by_item_statement(A, LU, B, LI, c, mutation="sides_exchanged")
    affected = _bits(Zt) != _bits(mutated)
    assert 0.1 < affected.mean() < 0.9
    assert not affected[:, 7].any() and not affected[11].any()
    # the check of the GPU tests, on the lists at full depth: the values of the unaffected logits pass,
    # every affected one is refused by itself
    users, values, _ = ac.expected_lists(mutated, n_users)
    for i in range(n_items):
        got = values[i][np.argsort(users[i])]  # by user
        differ = _bits(got) != _bits(Zt[i])
        np.testing.assert_array_equal(differ, affected[i])
    clean = np.flatnonzero(~affected.any(axis=1))
    assert 11 in clean
    ac.assert_lists(users[clean], values[clean], Zt, n_users, clean, None, "items without an affected logit")
    for i in np.flatnonzero(affected.any(axis=1))[:20]:
        with pytest.raises(AssertionError):
            ac.assert_lists(users[[i]], values[[i]], Zt, n_users, [i], None, f"item {i}")


def test_mutation_tie_broken_by_the_lower_user_index():
    n_items, n_users, k = 60, 70, 5
    A, LU, B, LI, c = (np.array(a) for a in ac.operands(n_items, n_users, k))
    A[40], LU[40] = A[12], LU[12]  # two identical user rows: a tie in every item's list
    Zt = ac.by_item_statement(A, LU, B, LI, c)
    assert ac.same_bytes(Zt[:, 40], Zt[:, 12])
    users, values, _ = ac.expected_lists(Zt, n_users)
    at = np.array([row.tolist().index(40) for row in users])
    assert (users[np.arange(n_items), at + 1] == 12).all(), "the higher index comes first"
    ac.assert_lists(users, values, Zt, n_users, None, None, "statement")
    K = 9
    got_users, got_values, _ = ac.expected_lists(Zt, K, mutation="lower_user_first")
    hit = np.flatnonzero(at < K)  # the items whose list reaches the tie
    assert 0 < hit.size < n_items
    others = np.setdiff1d(np.arange(n_items), hit)
    ac.assert_lists(got_users[others], got_values[others], Zt, K, others, None, "lists that do not reach the tie")
    for i in hit:
        with pytest.raises(AssertionError):
            ac.assert_lists(got_users[[i]], got_values[[i]], Zt, K, [i], None, f"item {i}")


def test_mutation_exclusion_list_read_at_the_user_s_offsets():
    n_items, n_users, k = 70, 9, 5  # (every user has offsets in an indptr of 71 entries)
    ops = ac.operands(n_items, n_users, k)
    Zt = ac.by_item_statement(*ops)
    M = np.random.default_rng(9).random((n_items, n_users)) < 0.2
    M[:n_users] = False  # the lists that the mutation reads: item 1 excludes user 1, the others nobody
    M[4], M[20], M[1, 1] = False, False, True
    M[20, 1] = True      # an item whose own list is what the mutation reads: it cannot tell
    indptr, users_of = pc.mask_csr(M)
    assert ac.same_bytes(ac.excluded_mask(indptr, users_of, n_items, n_users), M)
    wrong = ac.excluded_mask(indptr, users_of, n_items, n_users, mutation="excl_at_user_offsets")
    depth = n_users
    got = ac.expected_lists(Zt, depth, excluded=wrong)
    affected = np.flatnonzero((wrong != M).any(axis=1))
    clean = np.setdiff1d(np.arange(n_items), affected)
    assert 0 < affected.size and {1, 20} <= set(clean.tolist())
    ac.assert_lists(got[0][clean], got[1][clean], Zt, depth, clean, M, "unaffected items", got[2][clean])
    for i in affected:
        with pytest.raises(AssertionError):
            ac.assert_lists(got[0][[i]], got[1][[i]], Zt, depth, [i], M, f"item {i}", got[2][[i]])
    # an item whose own list is empty is affected too: it loses the user that lists itself
    assert 4 in affected and got[2][4] == n_users - 1


# --------------------------------------------------------------------------
# the host transposition of exclude
# --------------------------------------------------------------------------
def _against_scipy(E, n_users, n_items):
    from relevance_factorizationmachine_amd import recommend as rec
    got = rec.transposed_exclusions(rec._host_exclusions(E, n_users, n_items), n_items)
    T = sp.csr_matrix(E).T.tocsr()
    T.sum_duplicates()
    T.sort_indices()
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32
    np.testing.assert_array_equal(got[0], T.indptr)
    np.testing.assert_array_equal(got[1], T.indices)
    plain = ac.transpose_lists(*rec._host_exclusions(E, n_users, n_items), n_items)
    np.testing.assert_array_equal(got[0], plain[0])
    np.testing.assert_array_equal(got[1], plain[1])
    return got


def test_exclude_is_transposed_as_scipy_transposes_it():
    from relevance_factorizationmachine_amd import recommend as rec
    n_users, n_items = 7, 11
    rng = np.random.default_rng(3)
    M = rng.random((n_users, n_items)) < 0.3
    M[2] = False          # empty rows
    M[5] = False
    M[:, 4] = False       # an empty column
    _against_scipy(sp.csr_matrix(M.astype(np.float64)), n_users, n_items)
    full_row = M.copy()
    full_row[3] = True
    got = _against_scipy(sp.csr_matrix(full_row.astype(np.float64)), n_users, n_items)
    assert (np.diff(got[0]) >= 1).all()
    full_col = M.copy()
    full_col[:, 9] = True
    got = _against_scipy(sp.csr_matrix(full_col.astype(np.float64)), n_users, n_items)
    assert got[1][got[0][9]:got[0][10]].tolist() == list(range(n_users))
    # non-canonical input: unsorted columns and a pair stored twice
    rows = np.array([0, 0, 0, 1, 6, 6, 6])
    cols = np.array([9, 2, 9, 10, 0, 10, 3])
    loose = sp.csr_matrix((np.ones(7), cols, np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n_users))])),
                          shape=(n_users, n_items))
    assert not loose.has_canonical_format
    got = _against_scipy(loose, n_users, n_items)
    assert got[0][-1] == 6  # the repeated pair is one pair
    # the (indptr, indices) form, and nothing
    lists = pc.mask_csr(M)
    got = rec.transposed_exclusions(rec._host_exclusions(lists, n_users, n_items), n_items)
    np.testing.assert_array_equal(got[1], sp.csr_matrix(M.astype(np.float64)).T.tocsr().indices)
    assert rec.transposed_exclusions(None, n_items) is None
    empty = rec.transposed_exclusions(rec._host_exclusions(sp.csr_matrix((n_users, n_items)), n_users, n_items), n_items)
    assert empty[0].tolist() == [0] * (n_items + 1) and empty[1].size == 0
    with pytest.raises(ValueError, match="exclude has shape"):
        rec._host_exclusions(sp.csr_matrix((n_items, n_users)), n_users, n_items)


# --------------------------------------------------------------------------
# the ABI table and the Python surface
# --------------------------------------------------------------------------
TWINS = {"rfm_pair_topk_by_item": "rfm_pair_topk", "rfm_pair_ranks_by_item": "rfm_pair_ranks_n",
         "rfm_pair_order_by_item": "rfm_pair_order"}


def test_header_declares_the_new_entries_as_the_ctypes_table_has_them():
    """include/rfm_audience.h (which rfm_hip.h includes, once) against ``_lib.AUDIENCE_SIGNATURES``,
    argument by argument; each entry takes its forward twin's argument list with the ids, lists and
    outputs renamed (and ``raw`` after ``k``); the library exports the three and binds them."""
    import ctypes as C

    from relevance_factorizationmachine_amd import _lib
    main = open(os.path.join(ROOT, "include", "rfm_hip.h")).read()
    header = open(os.path.join(ROOT, "include", "rfm_audience.h")).read()
    assert main.count('#include "rfm_audience.h"') == 1 and main.count('#include "rfm_neighbours.h"') == 1
    declarations = r"^int32_t\s+(rfm_\w+)\s*\(([^)]*)\)\s*;"
    found = re.findall(declarations, re.sub(r"/\*.*?\*/", " ", header, flags=re.S), flags=re.M)
    assert [name for name, _ in found] == list(_lib.AUDIENCE_SIGNATURES) == list(TWINS)
    assert not set(_lib.AUDIENCE_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.NEIGHBOUR_SIGNATURES))
    kinds = {C.c_int32: "int32_t", C.c_int64: "int64_t"}
    lib = _lib.load()
    in_main = dict(re.findall(declarations, re.sub(r"/\*.*?\*/", " ", main, flags=re.S), flags=re.M))
    for name, params in found:
        params = [p.strip() for p in params.split(",")]
        want = ["pointer" if "*" in p else p.split()[0] for p in params]
        got = [kinds.get(t, "pointer") for t in _lib.AUDIENCE_SIGNATURES[name]]
        assert want == got, (name, want, got)
        assert getattr(lib, name).argtypes == _lib.AUDIENCE_SIGNATURES[name] and getattr(lib, name).restype is C.c_int32
        mine = re.sub(r"\s+", " ", ", ".join(params))
        for new, old in (("d_item_ids", "d_user_ids"), ("n_sel_items", "n_sel_users"), ("d_excl_users", "d_excl_items"),
                         ("d_tgt_users", "d_tgt_items"), ("d_out_users", "d_out_items"), ("d_out_values", "d_out_scores"),
                         ("int32_t k, int32_t raw", "int32_t k")):
            mine = mine.replace(new, old)
        assert mine == re.sub(r"\s+", " ", in_main[TWINS[name]]).strip(), f"{name} does not take {TWINS[name]}'s arguments"
    assert _lib.AUDIENCE_SIGNATURES["rfm_pair_ranks_by_item"] == _lib.SIGNATURES["rfm_pair_ranks_n"]
    assert _lib.AUDIENCE_SIGNATURES["rfm_pair_order_by_item"] == _lib.SIGNATURES["rfm_pair_order"]
    text = re.sub(r"\s*\n \*\s*", " ", header)
    assert "rfm_pair_geometry(n_sel_items, n_users, n_factors)" in text and "rfm_pair_order_geometry(n_users, depth)" in text
    assert "no query of its own is needed" in text


def test_model_methods_exist_with_the_issue_s_signatures():
    import inspect

    import relevance_factorizationmachine_amd as pkg
    tail = ["exclude", "new_items", "new_users"]
    for cls, lead in ((pkg.LogisticMatrixFactorization, ["self"]), (pkg.FactorizationMachines, ["self", "sides"])):
        names = lambda f: list(inspect.signature(getattr(cls, f)).parameters)  # noqa: E731
        assert names("recommend_users") == lead + ["k", "items"] + tail
        assert names("rank_users") == lead + ["items", "users"] + tail
        assert names("rank_audience") == lead + ["depth", "items"] + tail + ["workspace_bytes"]


def _folded(side, **arrays):
    return types.SimpleNamespace(side=side, **{n: np.zeros(s) for n, s in arrays.items()})


def test_operands_refuses_folded_rows_of_the_other_side_class_or_width():
    """The checks of ``operands(new_items=)`` run before anything touches the device, and are the
    errors ``new_users=`` raises: the other side and the other model class a TypeError, another factor
    count a ValueError."""
    from relevance_factorizationmachine_amd import recommend as rec
    mf = types.SimpleNamespace(n_factors=5)
    fm = types.SimpleNamespace(n_factors=5, n_features=40)
    rows_item, rows_user = _folded("item", rows=(3, 5), bias=(3,)), _folded("user", rows=(3, 5), bias=(3,))
    cols_item = _folded("item", w=(3,), V=(3, 5), A=(3, 8), L=(3,))
    cols_user = _folded("user", w=(3,), V=(3, 5), A=(3, 8), L=(3,))
    for model, kw, text in (
            (mf, dict(new_items=rows_user), "new_items takes the FoldedRows of fold_in_items"),
            (mf, dict(new_users=rows_item), "new_users takes the FoldedRows of fold_in_users"),
            (mf, dict(new_items=cols_item), "new_items takes the FoldedRows of fold_in_items"),
            (fm, dict(new_items=cols_user), "new_items of an FM model takes the FoldedColumns of its fold_in_items"),
            (fm, dict(new_users=cols_item), "new_users of an FM model takes the FoldedColumns of its fold_in_users"),
            (fm, dict(new_items=rows_item), "new_items of an FM model takes the FoldedColumns of its fold_in_items"),
            (mf, dict(new_users=rows_user, new_items=rows_user), "new_items takes the FoldedRows of fold_in_items")):
        with pytest.raises(TypeError, match=text):
            rec.operands(model, None, **kw)
    with pytest.raises(ValueError, match=r"folded rows of \(3, 4\) for a model of 5 factors"):
        rec.operands(mf, new_items=_folded("item", rows=(3, 4), bias=(3,)))
    with pytest.raises(ValueError, match=r"folded operands of \(3, 12\) for a model of 5 factors"):
        rec.operands(fm, None, new_items=_folded("item", w=(3,), V=(3, 5), A=(3, 12), L=(3,)))


def test_group_pairs_groups_by_item_for_this_direction():
    from relevance_factorizationmachine_amd import recommend as rec
    items, users = np.array([4, 0, 4, 4, 2]), np.array([9, 1, 3, 9, 0])
    sel, indptr, tgt, order = rec.group_pairs(items, users, 5, 10, ("items", "users"))
    assert sel.tolist() == [0, 2, 4] and indptr.tolist() == [0, 1, 2, 5] and tgt.tolist() == [1, 0, 3, 9, 9]
    assert items[order].tolist() == [0, 2, 4, 4, 4]
    with pytest.raises(ValueError, match="an item id lies outside 0..4"):
        rec.group_pairs(np.array([5]), np.array([0]), 5, 10, ("items", "users"))
    with pytest.raises(ValueError, match="a user id lies outside 0..9"):
        rec.group_pairs(np.array([0]), np.array([10]), 5, 10, ("items", "users"))
    with pytest.raises(ValueError, match="2 items for 1 users"):
        rec.group_pairs(np.array([0, 1]), np.array([1]), 5, 10, ("items", "users"))


# --------------------------------------------------------------------------
# the geometry of every GPU case list
# --------------------------------------------------------------------------
def test_geometry_of_the_bitwise_cases():
    """With the counts exchanged: the queries are items, the candidates users."""
    classes = set()
    for n_items, n_users, k in ac.BITWISE_CASES:
        g = pc.geometry(n_items, n_users, k)
        full, q = pc.kpad_class(k)
        assert (g["kpad"], g["chunks"], g["tail_quarter"]) == (pc.pad4(k), full + 1, q), g
        assert (g["user_tiles"], g["item_tiles"]) == (-(-n_items // pc.TILE), -(-n_users // pc.TILE)), g
        assert g["tiles_per_split"] == 1 and g["n_splits"] == g["item_tiles"]
        og = pc.order_geometry(n_users, n_users)
        assert (og["P"], og["pages"]) == (256, 1)
        classes.add((g["user_tiles"], g["item_tiles"]))
    assert classes == {(a, b) for a in (1, 2, 3) for b in (1, 2, 3)}
    assert {pc.kpad_class(k) for k in ac.EDGE_FACTORS + ac.BITWISE_FACTORS} == {(0, 1), (0, 2), (1, 1), (1, 2), (31, 8)}


@pytest.mark.parametrize("n_users", list(ac.WALK_USERS))
@pytest.mark.parametrize("n_sel", ac.WALK_SEL)
def test_geometry_of_the_walks(n_sel, n_users):
    for k in ac.WALK_FACTORS:
        g = pc.geometry(n_sel, n_users, k)
        assert (g["item_tiles"], g["tiles_per_split"], g["n_splits"], g["last_split_tiles"]) == ac.WALK_USERS[n_users]
        assert g["user_tiles"] == 33 and n_sel - 32 * pc.TILE in (pc.TILE, 1)
        assert g["last_split_tiles"] < g["tiles_per_split"] in (2, 3)
    assert n_users < 5000 and n_sel < 5000
    M = ac.walk_exclusions(n_users, ac.WALK_USERS[n_users][1])
    lo = ac.WALK_USERS[n_users][1] * pc.TILE
    assert M.shape == (ac.WALK_ITEMS, n_users) and M[ac.WALK_EMPTY_ITEM].all()
    assert M[ac.WALK_EMPTY_SPLIT_ITEM, lo:2 * lo].all() and M[ac.WALK_EMPTY_SPLIT_ITEM].sum() == lo


def test_walk_orders_are_separated_for_the_oracle_check():
    for n_users in ac.WALK_USERS:
        for k in ac.WALK_FACTORS:
            o = ac.by_item_oracle(*ac.operands(ac.WALK_ITEMS, n_users, k))
            share = pc.separated_share(o)
            print(f"walk {n_users} users k={k}: separated share {share:.4f}")
            assert share >= 0.99
