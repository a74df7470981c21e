"""Host half of the neighbour tests (no GPU): the long-double oracle of
neighbours_common.py against plain NumPy, the floor under its derived tolerances, the share of
separated positions of every order case, six mutations each caught by the checks the GPU tests go
through (and on the affected rows alone), the header's new entries against the ctypes table, and
the argument checks of recommend.py that need no device."""
import os
import re
import types

import numpy as np
import pytest
from scipy import sparse as sp

import neighbours_common as nc
import pair_tile_common as pc
from neighbours_common import LD

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDER_CASES = [(n, k) for n in nc.NEIGHBOUR_ROWS for k in nc.HOST_FACTORS]


def test_oracle_against_plain_numpy():
    for n, k in ((129, 5), (193, 37), (129, 400)):
        R = nc.rows(n, k)
        unit = R / np.linalg.norm(R, axis=1)[:, None]
        o = nc.oracle(R, "cosine")
        assert np.max(np.abs(o.z.astype(np.float64) - unit @ unit.T)) < 1e-12
        assert np.max(np.abs(nc.oracle(R, "dot").z.astype(np.float64) - R @ R.T)) < 1e-12 * k
        assert np.max(np.abs(np.diag(o.z).astype(np.float64) - 1.0)) < 1e-15
        norm, rows = nc.norms_ld(R)
        assert np.max(np.abs(norm.astype(np.float64) - np.linalg.norm(R, axis=1))) < 1e-12
        assert np.max(np.abs(rows.astype(np.float64) - unit)) < 1e-12


def test_oracle_gives_nan_to_rows_without_a_direction():
    k = 5
    R = nc.special_rows(k)
    _, unit = nc.norms_ld(R)
    names = dict(zip(nc.SPECIAL_ROWS, unit))
    for name in ("all zero", "a NaN", "an Inf", "1e200", "1e-200"):
        assert np.isnan(names[name]).all(), name
    assert names["a single non-zero"][k - 1] == -1 and not names["a single non-zero"][:k - 1].any()
    assert names["-0.0"][0] == 0 and np.signbit(names["-0.0"][0])
    o = nc.oracle(R, "cosine")
    undefined = np.isnan(unit).any(axis=1)
    assert np.isnan(o.z[undefined]).all() and np.isnan(o.z[:, undefined]).all()
    assert not np.isnan(o.z[~undefined][:, ~undefined]).any()


@pytest.mark.parametrize("k", nc.NORMALISE_FACTORS)
def test_floor_of_the_element_bound(k):
    """The float64 statement, on the factors as stored and shuffled, stays below half of E; so do the norms."""
    R = nc.rows(257, k)
    want_norm, want = nc.norms_ld(R)
    E = LD(nc.element_bound(k))
    shuffle = np.random.default_rng(k).permutation(k)
    for name, cols in (("natural", np.arange(k)), ("shuffled", shuffle)):
        out, norm = nc.normalise_statement(R[:, cols], k)
        pc.assert_within(out[:, :k], want[:, cols], E * np.abs(want[:, cols]), f"k={k} {name} rows", bound=0.5)
        pc.assert_within(norm, want_norm, E * want_norm, f"k={k} {name} norms", bound=0.5)


@pytest.mark.parametrize("metric", nc.METRICS)
@pytest.mark.parametrize("n,k", [(n, k) for n in nc.NEIGHBOUR_ROWS for k in (1,) + nc.NEIGHBOUR_FACTORS])
def test_floor_of_the_value_tolerance(n, k, metric):
    """The float64 statement of rows and tile, factors in natural and in shuffled order, stays below
    half of the cosine's (dot product's) tolerance on every case of the GPU tests."""
    R = nc.rows(n, k)
    o = nc.oracle(R, metric)
    rows = nc.normalise_statement(R, k)[0][:, :k] if metric == "cosine" else R
    zero = np.zeros(n)
    for name, order in (("natural", None), ("shuffled", np.random.default_rng(n + k).permutation(k))):
        z = pc.pair_float64(rows, zero, rows, zero, 0.0, order)
        pc.assert_within(z, o.z, o.tol_z, f"{metric} n={n} k={k} {name}", bound=0.5)


@pytest.mark.parametrize("metric", nc.METRICS)
@pytest.mark.parametrize("n,k", ORDER_CASES)
def test_order_cases_are_separated(n, k, metric):
    share = pc.separated_share(nc.oracle(nc.rows(n, k), metric), nc.self_mask(n))
    print(f"separated share n={n} k={k} {metric}: {share:.4f}")
    assert share >= 0.99


def test_one_factor_is_an_exact_tie_case():
    o = nc.oracle(nc.rows(129, 1), "cosine")
    assert set(np.unique(o.z.astype(np.float64)).tolist()) == {-1.0, 1.0}
    assert pc.separated_share(o, nc.self_mask(129)) < 0.05
    out, _ = nc.normalise_statement(nc.rows(129, 1), 1)
    assert set(np.unique(out[:, 0]).tolist()) == {-1.0, 1.0} and not out[:, 1:].any()


# --------------------------------------------------------------------------
# mutations
# --------------------------------------------------------------------------
def _rows_fail(out, norm, R, k, rows):
    """assert_normalised passes on the rows outside ``rows`` and refuses each row of ``rows`` by itself."""
    others = np.setdiff1d(np.arange(R.shape[0]), rows)
    nc.assert_normalised(out[others], norm[others], R[others], k, "unaffected rows")
    for r in rows:
        try:
            nc.assert_normalised(out[[r]], norm[[r]], R[[r]], k, f"affected row {r}")
        except AssertionError:
            continue
        return False
    return True


@pytest.mark.parametrize("k", (5, 65, 129))
def test_statement_passes_the_checks_it_is_mutated_against(k):
    R = np.vstack([nc.rows(9, k), nc.special_rows(k)])
    out, norm = nc.normalise_statement(R, k)
    nc.assert_normalised(out, norm, R, k, f"k={k}")


@pytest.mark.parametrize("mutation", ("squared_norm", "l1_norm"))
def test_mutation_wrong_norm(mutation):
    k = 37
    R = np.array(nc.rows(9, k))
    R[4] = 0.0
    R[4, 3] = 1.0  # the one row whose squared norm, L1 norm and norm agree: it must pass
    out, norm = nc.normalise_statement(R, k, mutation)
    assert _rows_fail(out, norm, R, k, np.setdiff1d(np.arange(9), [4]))


@pytest.mark.parametrize("k", (1, 65, 129))
def test_mutation_sum_drops_the_last_factor(k):
    R = np.array(nc.rows(9, k))
    R[2, k - 1] = 0.0  # a row whose last factor is zero cannot tell
    out, norm = nc.normalise_statement(R, k, "drops_last_factor")
    assert _rows_fail(out, norm, R, k, np.setdiff1d(np.arange(9), [2]))
    # at any other k % 64 the mutation is the statement itself
    for other in (5, 64, 66):
        a, b = nc.normalise_statement(nc.rows(9, other), other, "drops_last_factor"), nc.normalise_statement(nc.rows(9, other), other)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_mutation_zeros_for_a_row_without_a_direction():
    k = 5
    R = np.vstack([nc.rows(4, k), nc.special_rows(k)])
    out, norm = nc.normalise_statement(R, k, "zero_rows_are_zero")
    undefined = 4 + np.array([nc.SPECIAL_ROWS.index(s) for s in ("all zero", "a NaN", "an Inf", "1e200", "1e-200")])
    assert _rows_fail(out, norm, R, k, undefined)


def _lists_fail(ids, values, o, K, sel, excluded, rows):
    """assert_lists passes on the queries outside ``rows`` and refuses each query of ``rows`` by itself."""
    sel = np.asarray(sel)
    keep = ~np.isin(np.arange(len(sel)), rows)
    if keep.any():
        nc.assert_lists(ids[keep], values[keep], o, K, sel[keep], excluded, "unaffected queries")
    for q in rows:
        try:
            nc.assert_lists(ids[[q]], values[[q]], o, K, sel[[q]], excluded, f"affected query {q}")
        except AssertionError:
            continue
        return False
    return True


@pytest.mark.parametrize("metric", nc.METRICS)
@pytest.mark.parametrize("K", nc.NEIGHBOUR_K)
def test_statement_lists_pass_and_list_mutations_are_caught(metric, K):
    n, k = 129, 5
    R = nc.rows(n, k)
    o, mask = nc.oracle(R, metric), nc.self_mask(n)
    sel = np.arange(n)
    ids, values = nc.lists_statement(R, K, metric)
    nc.assert_lists(ids, values, o, K, sel, mask, f"{metric} K={K}")
    # self not excluded: cosine -- every query is its own best neighbour; dot -- the queries whose
    # own squared norm is among their K largest products
    ids, values = nc.lists_statement(R, K, metric, mutation="self_not_excluded")
    hit = np.flatnonzero((ids == sel[:, None]).any(axis=1))
    assert hit.size == n if metric == "cosine" else hit.size > 0
    assert _lists_fail(ids, values, o, K, sel, mask, hit)
    # the values through the sigmoid: every query
    ids, values = nc.lists_statement(R, K, metric, mutation="sigmoid_values")
    assert _lists_fail(ids, values, o, K, sel, mask, sel)


def test_include_self_puts_self_first_with_cosine_one():
    n, k = 129, 37
    R = nc.rows(n, k)
    sel = nc.selection(n)
    ids, values = nc.lists_statement(R, 9, "cosine", sel, include_self=True)
    assert (ids[:, 0] == sel).all()
    o = nc.oracle(R, "cosine")
    nc.assert_lists(ids, values, o, 9, sel, None, "include_self")
    assert np.all(np.abs(values[:, 0].astype(LD) - 1) <= o.tol_z[sel, sel])


# --------------------------------------------------------------------------
# the ABI table and the Python checks that need no device
# --------------------------------------------------------------------------
def test_header_declares_the_new_entries_as_the_ctypes_table_has_them():
    """include/rfm_neighbours.h (which rfm_hip.h includes where the catalogue entries stand) against
    ``_lib.NEIGHBOUR_SIGNATURES``, argument by argument; the library exports both and binds them."""
    import ctypes as C

    from relevance_factorizationmachine_amd import _lib
    main = open(os.path.join(ROOT, "include", "rfm_hip.h")).read()
    header = open(os.path.join(ROOT, "include", "rfm_neighbours.h")).read()
    assert main.count('#include "rfm_neighbours.h"') == 1
    declarations = r"^int32_t\s+(rfm_\w+)\s*\(([^)]*)\)\s*;"
    found = re.findall(declarations, re.sub(r"/\*.*?\*/", " ", header, flags=re.S), flags=re.M)
    assert [name for name, _ in found] == list(_lib.NEIGHBOUR_SIGNATURES) == ["rfm_pair_topk_raw", "rfm_rows_normalise"]
    assert not set(_lib.NEIGHBOUR_SIGNATURES) & set(_lib.SIGNATURES)
    kinds = {C.c_int32: "int32_t", C.c_int64: "int64_t"}
    lib = _lib.load()
    for name, params in found:
        params = [p.strip() for p in params.split(",")]
        want = ["pointer" if "*" in p else p.split()[0] for p in params]
        got = [kinds.get(t, "pointer") for t in _lib.NEIGHBOUR_SIGNATURES[name]]
        assert want == got, (name, want, got)
        assert getattr(lib, name).argtypes == _lib.NEIGHBOUR_SIGNATURES[name] and getattr(lib, name).restype is C.c_int32
    topk = dict(re.findall(declarations, re.sub(r"/\*.*?\*/", " ", main, flags=re.S), flags=re.M))["rfm_pair_topk"]
    norm = lambda s: re.sub(r"\s+", " ", s).replace("d_out_values", "d_out_scores")  # noqa: E731
    assert norm(dict(found)["rfm_pair_topk_raw"]) == norm(topk), "the raw entry takes rfm_pair_topk's arguments"
    assert _lib.NEIGHBOUR_SIGNATURES["rfm_pair_topk_raw"] == _lib.SIGNATURES["rfm_pair_topk"]
    # the citation paragraph: where the vectors come from, and that the reference has no counterpart
    text = re.sub(r"\s*\n \*\s*", " ", header)
    assert "src/fm.py:114-133" in text and "src/mf.py:136-170" in text and "no counterpart" in text


def test_check_neighbours_refusals():
    from relevance_factorizationmachine_amd import recommend as rec
    n = 7
    for k in (0, 65, -1):
        with pytest.raises(ValueError, match="outside 1..64"):
            rec.check_neighbours(n, k)
    with pytest.raises(ValueError, match="neither 'cosine' nor 'dot'"):
        rec.check_neighbours(n, 3, metric="euclid")
    with pytest.raises(ValueError, match="an item id lies outside 0..6"):
        rec.check_neighbours(n, 3, ids=[0, 7])
    with pytest.raises(ValueError, match="a user id lies outside 0..2"):
        rec.check_neighbours(n, 3, ids=[3], n_queries=3, what="users")
    with pytest.raises(ValueError, match="1-d array of integer ids"):
        rec.check_neighbours(n, 3, ids=[0.5])
    with pytest.raises(ValueError, match="include_self"):
        rec.check_neighbours(n, 3, include_self=True, n_queries=3)
    with pytest.raises(ValueError, match="exclude has shape"):
        rec.check_neighbours(n, 3, exclude=sp.csr_matrix((n, n + 1)))
    with pytest.raises(ValueError, match="exclude has shape"):
        rec.check_neighbours(n, 3, exclude=sp.csr_matrix((n, n)), n_queries=3)
    k, sel, excl = rec.check_neighbours(n, 64, ids=[6, 0, 6], include_self=True)
    assert k == 64 and sel.dtype == np.int32 and sel.tolist() == [6, 0, 6] and excl is None
    k, sel, excl = rec.check_neighbours(n, 1, n_queries=3)
    assert sel is None and excl is None  # rows of another table have no self


def test_self_is_merged_into_the_exclusion_lists():
    from relevance_factorizationmachine_amd import recommend as rec
    n = 6
    indptr, items = rec.check_neighbours(n, 3)[2]
    assert indptr.dtype == np.int64 and items.dtype == np.int32
    assert indptr.tolist() == list(range(n + 1)) and items.tolist() == list(range(n))
    M = np.zeros((n, n), dtype=bool)
    M[0, [1, 5]] = True       # self goes in front
    M[2, [0, 2, 4]] = True    # self is listed already
    M[5, [0, 1]] = True       # self goes behind
    M[3, :] = True
    indptr, items = rec.check_neighbours(n, 3, exclude=sp.csr_matrix(M))[2]
    want = pc.mask_csr(M | np.eye(n, dtype=bool))
    assert indptr.tolist() == want[0].tolist() and items.tolist() == want[1].tolist()
    same = rec.check_neighbours(n, 3, exclude=pc.mask_csr(M))[2]
    assert same[0].tolist() == indptr.tolist() and same[1].tolist() == items.tolist()
    assert rec.check_neighbours(n, 3, exclude=sp.csr_matrix(M), include_self=True)[2][1].tolist() == pc.mask_csr(M)[1].tolist()


def _folded(side, **arrays):
    return types.SimpleNamespace(side=side, **{n: np.zeros(s) for n, s in arrays.items()})


def test_folded_queries_refusals():
    from relevance_factorizationmachine_amd import recommend as rec
    mf = types.SimpleNamespace(n_factors=5)
    fm = types.SimpleNamespace(n_factors=5, n_features=40)
    rows_item, rows_user = _folded("item", rows=(3, 5), bias=(3,)), _folded("user", rows=(3, 5), bias=(3,))
    cols_item = _folded("item", w=(3,), V=(3, 5), A=(3, 8), L=(3,))
    cols_user = _folded("user", w=(3,), V=(3, 5), A=(3, 8), L=(3,))
    assert rec.folded_queries(mf, "item", rows_item) is rows_item.rows
    assert rec.folded_queries(mf, "user", rows_user) is rows_user.rows
    assert rec.folded_queries(fm, "item", cols_item) is cols_item.A
    assert rec.folded_queries(fm, "user", cols_user) is cols_user.A
    for model, side, folded, text in (
            (mf, "item", rows_user, "new_items takes the FoldedRows of fold_in_items"),        # the other side
            (mf, "user", rows_item, "new_users takes the FoldedRows of fold_in_users"),
            (mf, "item", cols_item, "new_items takes the FoldedRows of fold_in_items"),        # the other class
            (fm, "item", cols_user, "new_items of an FM model takes the FoldedColumns of its fold_in_items"),
            (fm, "user", cols_item, "new_users of an FM model takes the FoldedColumns of its fold_in_users"),
            (fm, "user", rows_user, "new_users of an FM model takes the FoldedColumns of its fold_in_users"),
            (mf, "item", object(), "new_items takes the FoldedRows")):
        with pytest.raises(TypeError, match=text):
            rec.folded_queries(model, side, folded)
    with pytest.raises(ValueError, match=r"folded rows of \(3, 4\) for a model of 5 factors"):
        rec.folded_queries(mf, "item", _folded("item", rows=(3, 4), bias=(3,)))
    with pytest.raises(ValueError, match=r"folded operands of \(3, 12\) for a model of 5 factors"):
        rec.folded_queries(fm, "user", _folded("user", w=(3,), V=(3, 5), A=(3, 12), L=(3,)))


def test_model_methods_exist_with_the_issue_s_signatures():
    import inspect

    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import recommend as rec
    common = ["metric", "exclude", "include_self"]
    for cls, lead in ((pkg.LogisticMatrixFactorization, ["self", "k"]), (pkg.FactorizationMachines, ["self", "sides", "k"])):
        for side in ("items", "users"):
            names = list(inspect.signature(getattr(cls, f"similar_{side}")).parameters)
            assert names == lead + [side] + common + [f"new_{side}"], names
            assert "factor space only" in " ".join(getattr(cls, f"similar_{side}").__doc__.split())
    names = list(inspect.signature(rec.neighbours).parameters)
    assert names[:9] == ["rt", "R", "n_factors", "k", "ids", "metric", "exclude", "include_self", "queries"]
    assert list(inspect.signature(rec.normalised).parameters) == ["rt", "M", "n_factors"]
