"""The test infrastructure of MF fold-in (fold_in_common.py) and the host half of the feature, checked
without a GPU before any device result is held to them: the tolerance floor, the oracle against the
reference's own sequential batch, four mutations of the rule, the grouping and the order array that
``fold_in_users`` / ``fold_in_items`` hand the kernel, their argument checks, and the launch shape
``rfm_mf_fold_geometry`` reports at every kernel class.

The tests of the oracle itself (the floor, the case list, the clip case, rows at once, the reference
anchor, the mutations: eleven cases) call fold_in_common.py alone and so pass on the code before
fold-in as well; they check the yardstick, not the feature.  The grouping, the argument checks, the
geometry of the 19 classes and the entry points' bad arguments fail there: the functions do not
exist."""
import ctypes as C
import types

import numpy as np
import pytest

import fold_in_common as fc
import mf_step_common as ms
from oracle import cpu_ref

LD = np.longdouble


# --------------------------------------------------------------------------
# the tolerance floor
# --------------------------------------------------------------------------
def test_tolerance_floor():
    """f64 with the dot product summed backwards against the oracle, over every case: the floor the
    module's docstring states, and 64 times it is the tolerance."""
    rows = bias = 0.0
    for case in list(fc.fold_cases().values()) + [fc.grid_case(ms.ASSUMED_CUS)]:
        r, b = fc.floor_of(case)
        rows, bias = max(rows, r), max(bias, b)
    floor = max(rows, bias)
    print(f"floor: rows {rows:.3e}, biases {bias:.3e}")
    assert floor <= fc.FOLD_FLOOR <= 1.05 * floor  # the constant is the measured figure, not a looser one
    assert fc.FOLD_TOL == min(64 * fc.FOLD_FLOOR, 1e-11)


def test_case_list_covers_what_it_names():
    cases = fc.fold_cases()
    assert {ms.shape_class(c.k) for n, c in cases.items() if n.startswith("shape-")} == set(ms.CLASS_RANGE)
    d = fc.DEPTH
    for name, case in cases.items():
        if name.startswith("shape-"):
            lpr = ms.shape_class(case.k)[0]
            assert {0, 1, d - 1, d, d + 1, 2 * d - 1, 2 * d, 2 * d + 1} <= set(case.lengths.tolist())
            assert case.n_passes == 2 and (fc.LONG_CHAIN in case.lengths) == (lpr == 4)
            if lpr <= 8:  # every row of the case in one wavefront
                assert case.n_new <= 64 // lpr
        assert (np.sort(case.order) == np.arange(case.n_new)).all()
        assert (np.diff(case.lengths[case.order]) <= 0).all()
    assert {c.n_passes for n, c in cases.items() if n.startswith("passes")} == {0, 1, 2, 3}
    for k in fc.COUNT_KS:
        gpb = fc.rows_per_workgroup(k)
        assert {c.n_new for n, c in cases.items() if n.startswith("count") and c.k == k} == {1, gpb - 1, gpb, gpb + 1}
    special = cases["special-k7"]
    twice = special.chains[0]
    assert twice[1] == twice[2] == twice[4] and all(5 in c for c in special.chains) and special.clip
    assert any(0 in c for c in special.chains) and any(1 in c for c in special.chains)
    grid = fc.grid_case(ms.ASSUMED_CUS)
    assert grid.n_new == 131072 + 37 and set(grid.lengths.tolist()) == {0, 1, 2} and grid.with_init


def test_clip_case_saturates_on_both_sides():
    case = fc.fold_cases()["special-k7"]
    F, fb = case.fixed()
    assert fb[0] == 900.0 and fb[1] == -900.0
    x, c = fc.fold_row([0], [1.0], F, fb, np.zeros(7), 0.0, 1)
    err = 1 - 1 / (1 + np.exp(LD(-700)))  # the logit is clipped at +700, not 900.4
    assert c == LD(0) - LD(ms.LR) * (-err) and x[0] == -LD(ms.LR) * (-err * LD(F[0, 0]))
    _, c = fc.fold_row([1], [1.0], F, fb, np.zeros(7), 0.0, 1)
    assert c == LD(ms.LR) * (1 - 1 / (1 + np.exp(LD(700))))


def test_rows_at_once_equal_row_by_row():
    """The oracle's two forms: all rows step by step, and one row example by example."""
    for name in ("shape-k7", "special-init-k130", "passes3-k33"):
        case = fc.fold_cases()[name]
        want = fc.oracle(case)
        F, fb = case.fixed()
        x0, c0 = case.start()
        ry, ptr = case.ry(), case.row_ptr
        for r in range(case.n_new):
            sl = slice(ptr[r], ptr[r + 1])
            x, c = fc.fold_row(case.ids[sl], ry[sl], F, fb, x0[r], c0[r], case.n_passes)
            # the same operations on the same operands; only the dot product's sum of k terms may round
            # differently, by at most k units in the last place of a long double per step
            tol = 64 * case.k * np.finfo(LD).eps
            assert np.abs(x - want[0][r]).max() <= tol * max(np.abs(x).max(), 1e-300)
            assert abs(c - want[1][r]) <= tol * max(abs(c), ms.LR)
        if not case.with_init:
            empty = np.flatnonzero(case.lengths == 0)
            assert empty.size and not want[0][empty].any() and not want[1][empty].any()


# --------------------------------------------------------------------------
# the reference anchor
# --------------------------------------------------------------------------
@pytest.mark.parametrize("k,seed", [(3, 0), (16, 1), (130, 2)])
def test_user_side_is_the_reference_batch_on_the_grown_model(k, seed):
    """User side, one pass, globally distinct items: the folded rows are the user rows after the
    reference's sequential batch on the model grown by the new users' starting rows."""
    rng = np.random.default_rng(seed)
    n_old, n_items, n_new = 5, 60, 6
    lengths = [0, 1, 4, 9, 17, 23]
    items = rng.permutation(n_items)[: sum(lengths)]
    chains = np.split(items, np.cumsum(lengths)[:-1])
    P, Q, bu, bi = cpu_ref.mf_init(seed, n_old, n_items, k)
    x0, c0 = rng.uniform(-1, 1, size=(n_new, k)), rng.normal(scale=0.1, size=n_new)
    y = (rng.random(len(items)) < 0.5).astype(np.float64)
    p = rng.uniform(0.1, 1.0, size=len(items)) ** 0.5
    new = np.repeat(np.arange(n_new), lengths)
    pos = np.concatenate([np.arange(n) for n in lengths])
    take = np.lexsort((new, pos))  # the users' examples interleaved in the batch
    pairs = np.stack([n_old + new, items], axis=1)[take]
    grown = [np.concatenate([P, x0]), Q.copy(), np.concatenate([bu, c0]), bi.copy()]
    cpu_ref.mf_sgd_batch(pairs, y[take], p[take], *grown, ms.B0, ms.LR, ms.REG)
    ptr = np.concatenate([[0], np.cumsum(lengths)])
    worst = 0.0
    for r in range(n_new):
        sl = slice(ptr[r], ptr[r + 1])
        x, c = fc.fold_row(chains[r], (y / p)[sl], Q, bi, x0[r], c0[r], 1)
        worst = max(worst, fc.assert_within((grown[0][n_old + r][None], grown[2][n_old + r][None]),
                                            (x[None], np.asarray([c])), fc.FOLD_TOL, f"user {r}"))
    print(f"anchor k{k} {worst:.3e}")
    np.testing.assert_array_equal(grown[0][:n_old], P)  # the batch touched no other user


# --------------------------------------------------------------------------
# mutations: the oracle catches each on the affected row alone
# --------------------------------------------------------------------------
@pytest.mark.parametrize("mutation", ["stale", "moves_fixed", "drops_last", "example_major"])
def test_oracle_catches_a_mutation_on_its_row_alone(mutation):
    case = fc.fold_cases()["special-k7"]
    want = fc.oracle(case)
    F, fb = case.fixed()
    x0, c0 = case.start()
    ry, ptr = case.ry(), case.row_ptr
    victim = 4  # eleven examples, three passes, a fixed row named twice in succession
    got = [np.asarray(want[0], dtype=np.float64), np.asarray(want[1], dtype=np.float64)]
    sl = slice(ptr[victim], ptr[victim + 1])
    x, c = fc.fold_row(case.ids[sl], ry[sl], F, fb, x0[victim], c0[victim], case.n_passes, mutation=mutation)
    got[0][victim], got[1][victim] = x, c
    rows = ms.row_distance(got[0], want[0]).max(axis=1)
    assert rows[victim] > 1e-4, (mutation, float(rows[victim]))  # thirteen orders above the tolerance
    assert (np.delete(rows, victim) <= fc.FOLD_TOL).all()
    with pytest.raises(AssertionError):
        fc.assert_within(got, want, fc.FOLD_TOL, mutation)
    # the unmutated row passes
    x, c = fc.fold_row(case.ids[sl], ry[sl], F, fb, x0[victim], c0[victim], case.n_passes)
    got[0][victim], got[1][victim] = x, c
    fc.assert_within(got, want, fc.FOLD_TOL, "unmutated")


# --------------------------------------------------------------------------
# grouping, order array and argument checks of the Python entry (no device)
# --------------------------------------------------------------------------
def test_grouping_of_interleaved_input_is_stable():
    from relevance_factorizationmachine_amd.fold import fold_examples
    case = fc.fold_cases()["shape-k7"]
    for side, col in (("user", 0), ("item", 1)):
        for interleaved in (False, True):
            data = case.data(side, interleaved)
            if interleaved:
                assert (np.diff(data["features"][:, col]) < 0).any()  # the input is not grouped
            row_ptr, ids, ry, order = fold_examples(data, case.n_new, case.n_fixed, col, case.n_passes)
            assert row_ptr.dtype == np.int64 and ids.dtype == np.int32 and ry.dtype == np.float64 and order.dtype == np.int32
            np.testing.assert_array_equal(row_ptr, case.row_ptr)
            np.testing.assert_array_equal(ids, case.ids)
            np.testing.assert_array_equal(ry, case.ry())  # label / propensity, the division fit() does
            np.testing.assert_array_equal(order, case.order)
    # descending example count, stable: equal counts keep their row order
    data = {"features": np.array([[2, 0], [0, 1], [2, 1], [3, 2], [0, 0], [4, 1], [4, 0]]), "labels": np.ones(7),
            "pscores": np.full(7, 0.5)}
    row_ptr, ids, ry, order = fold_examples(data, 6, 3, 0, 1)
    assert row_ptr.tolist() == [0, 2, 2, 4, 5, 7, 7] and ids.tolist() == [1, 0, 0, 1, 2, 1, 0]
    assert order.tolist() == [0, 2, 4, 3, 1, 5] and (ry == 2.0).all()
    # integer labels divide as floats
    data["labels"] = np.ones(7, dtype=np.int64)
    assert (fold_examples(data, 6, 3, 0, 1)[2] == 2.0).all()


def test_argument_checks_need_no_device():
    from relevance_factorizationmachine_amd import recommend as rec
    from relevance_factorizationmachine_amd.fold import fold_examples
    from relevance_factorizationmachine_amd.mf import FoldedRows, LogisticMatrixFactorization
    good = {"features": np.array([[0, 1], [1, 2]]), "labels": np.ones(2), "pscores": np.ones(2)}
    fold_examples(good, 2, 3, 0, 1)
    fold_examples(good, 2, 3, 0, 0)
    empty = {"features": np.zeros((0, 2), dtype=np.int64), "labels": np.zeros(0), "pscores": np.zeros(0)}
    row_ptr, ids, ry, order = fold_examples(empty, 3, 3, 0, 1)
    assert row_ptr.tolist() == [0, 0, 0, 0] and ids.size == ry.size == 0 and order.tolist() == [0, 1, 2]
    with pytest.raises(IndexError):
        fold_examples(good, 1, 3, 0, 1)      # new index 1 of one new user
    with pytest.raises(IndexError):
        fold_examples(good, 2, 2, 0, 1)      # item 2 of two items
    with pytest.raises(IndexError):
        fold_examples({**good, "features": np.array([[0, 1], [-1, 2]])}, 2, 3, 0, 1)
    with pytest.raises(IndexError):
        fold_examples(good, 2, 2, 1, 1)      # the item side: new index 2 of two new items
    with pytest.raises(ValueError):
        fold_examples(good, 2, 3, 0, -1)
    with pytest.raises(ValueError):
        fold_examples({**good, "labels": np.ones(3)}, 2, 3, 0, 1)
    with pytest.raises(ValueError):
        fold_examples({**good, "pscores": np.ones(1)}, 2, 3, 0, 1)
    with pytest.raises(ValueError):
        fold_examples({**good, "features": np.array([0, 1])}, 2, 3, 0, 1)
    # a model without b: the AttributeError predict() gives, before anything touches the device
    unfitted = types.SimpleNamespace(_rt=None)
    with pytest.raises(AttributeError, match="has no attribute 'b'"):
        LogisticMatrixFactorization._fold_in(unfitted, 0, good, 2, 1, None)
    # new_users on an FM model
    fm = types.SimpleNamespace(n_features=5, n_factors=4)
    folded = FoldedRows("user", np.zeros((2, 4)), np.zeros(2), None)
    with pytest.raises(TypeError, match="Sides"):
        rec.operands(fm, sides=None, new_users=folded)
    mf = types.SimpleNamespace(n_factors=4, b=0.1)
    with pytest.raises(TypeError):
        rec.operands(mf, new_users=FoldedRows("item", np.zeros((2, 4)), np.zeros(2), None))
    with pytest.raises(ValueError):
        rec.operands(mf, new_users=FoldedRows("user", np.zeros((2, 5)), np.zeros(2), None))
    with pytest.raises(TypeError):
        LogisticMatrixFactorization._append(mf, folded, "item", None, None)


# --------------------------------------------------------------------------
# the launch shape the library reports
# --------------------------------------------------------------------------
@pytest.mark.parametrize("cls", list(ms.CLASS_RANGE))
def test_geometry_at_every_class(cls):
    lpr, vec, nc = cls
    for k in ms.CLASS_RANGE[cls]:
        for n_new in (1, 256 // lpr + 1, 1 << 22):
            g = fc.geometry(n_new, k)
            assert (g["lpr"], g["vec"], g["nc"]) == cls, (k, g)
            assert g["rows"] == 256 // lpr == fc.rows_per_workgroup(k)
            assert g["depth"] == fc.DEPTH
            assert g["grid"] == min(-(-n_new // g["rows"]), ms.ASSUMED_CUS * fc.GRID_PER_CU)
    assert fc.geometry(0, ms.CLASS_RANGE[cls][0])["grid"] == 0


def test_entry_points_reject_bad_arguments():
    from relevance_factorizationmachine_amd import _lib
    lib = _lib.load()
    out = np.zeros(6, dtype=np.int32)
    for n_new, k, ptr in ((1, 0, out.ctypes.data), (1, ms.MAX_FACTORS + 1, out.ctypes.data), (-1, 4, out.ctypes.data),
                          (1, 4, None)):
        assert lib.rfm_mf_fold_geometry(None, n_new, k, ptr) == _lib.RFM_ERR_BAD_ARG
        assert _lib.last_error()
    # without a context nothing is launched: a null ctx is a bad argument like any other null pointer
    one = C.c_void_p(out.ctypes.data)
    assert lib.rfm_mf_fold_in(None, one, one, one, one, 1, one, one, 1, 0.0, 4, 0.1, 0.1, 1, one, one) == _lib.RFM_ERR_BAD_ARG
    assert "ctx" in _lib.last_error()
