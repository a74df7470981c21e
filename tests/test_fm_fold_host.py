"""The test infrastructure of FM fold-in (fm_fold_common.py) and the host half of the feature, checked
without a GPU before any device result is held to them: the tolerance floor and the step-size rule,
the oracle against the reference's own batch step on the grown model, four mutations of the rule, the
grouping and the order array that ``fold_in_users`` / ``fold_in_items`` hand the kernel, their
argument checks, the flows' ranking gaps, and the launch shape ``rfm_fm_fold_geometry`` reports at
every kernel class.

The tests of the oracle itself (the floor, the case list, the clip case, the anchor, the mutations, the
gaps) call fm_fold_common.py and the CPU oracle alone; they check the yardstick, not the feature.  The
grouping, the argument checks, the geometry of the 19 classes and the entry points' bad arguments fail
on the code before FM fold-in: the functions do not exist."""
import ctypes as C
import types

import numpy as np
import pytest
import scipy.sparse as sp

import fm_fold_common as fc
import mf_step_common as ms
from oracle import cpu_ref

LD = np.longdouble


# --------------------------------------------------------------------------
# the tolerance floor and the step-size rule
# --------------------------------------------------------------------------
def test_tolerance_floor_and_step_size_rule():
    """f64 with every sum in the opposite order against the oracle, over every case: the floor the
    module states, and 64 times it is the tolerance.  Every case's lr keeps a pass from amplifying."""
    rows = bias = 0.0
    for case in fc.fold_cases().values():
        assert case.lr * case.step_bound() <= 0.5 and 0 < case.lr <= fc.LR_CAP, case.name
        if case.lengths.sum():
            assert 2 * case.lr * case.step_bound() > 0.5 or case.lr == fc.LR_CAP, case.name  # (the largest such power of two)
        r, b = fc.floor_of(case)
        rows, bias = max(rows, r), max(bias, b)
    floor = max(rows, bias)
    print(f"floor: factor rows {rows:.3e}, weights {bias:.3e}")
    assert floor <= fc.FMFOLD_FLOOR <= 1.05 * floor  # the constant is the measured figure, not a looser one
    assert fc.FMFOLD_TOL == min(64 * fc.FMFOLD_FLOOR, 1e-11)
    assert fc.GPU_MAX_SEEN is None or fc.GPU_MAX_SEEN <= fc.FMFOLD_TOL


def test_case_list_covers_what_it_names():
    cases = fc.fold_cases()
    assert {ms.shape_class(c.k) for n, c in cases.items() if n.startswith("shape-")} == set(ms.CLASS_RANGE)
    assert any(c.k % 4 for c in cases.values()) and any(c.k % 4 == 0 for c in cases.values())
    for name, case in cases.items():
        gpb = fc.groups(case.k)
        if name.startswith("shape-"):
            lpr = ms.shape_class(case.k)[0]
            assert {0, 1, gpb - 1, gpb, gpb + 1, 2 * gpb + 1} <= set(case.lengths.tolist())
            assert case.n_passes == 2 and (fc.LONG_ROW in case.lengths) == (lpr == 4)
        assert (np.sort(case.order) == np.arange(case.n_new)).all()
        assert (np.diff(case.lengths[case.order]) <= 0).all()
        assert case.ids.size == 0 or (0 <= case.ids.min() and case.ids.max() < case.n_fixed)
    assert {c.n_passes for n, c in cases.items() if n.startswith("passes")} == {0, 1, 2, 3}
    grid = fc.ASSUMED_GRID
    assert grid == fc.geometry(1 << 20, 8)["grid"] == 2048
    for k in fc.COUNT_KS:
        counted = [c for n, c in cases.items() if n.startswith("count") and c.k == k]
        assert {c.n_new for c in counted} == {1, grid - 1, grid, grid + 1}
        assert all(set(c.lengths.tolist()) <= {0, 1, 2} for c in counted)
    special = cases["special-k7"]
    twice = special.chains[0]
    assert twice[1] == twice[2] == twice[4] and all(5 in c for c in special.chains) and special.clip
    assert any(0 in c for c in special.chains) and any(1 in c for c in special.chains)


def test_clip_case_saturates_on_both_sides():
    case = fc.fold_cases()["special-k7"]
    F, fL = case.fixed()
    g, l = case.feature_sums()
    assert fL[0] == 900.0 and fL[1] == -900.0
    lr = LD(case.lr)
    nu, om = fc.fold_row([0], [1.0], F, fL, g[0], l[0], fc.C0, np.zeros(7), 0.0, 1, case.lr)
    err = 1 - 1 / (1 + np.exp(LD(-700)))  # the logit is clipped at +700, not 900-odd
    assert om == lr * err and nu[0] == lr * (err * (LD(g[0, 0]) + LD(F[0, 0])))
    _, om = fc.fold_row([1], [1.0], F, fL, g[0], l[0], fc.C0, np.zeros(7), 0.0, 1, case.lr)
    assert om == lr * (1 - 1 / (1 + np.exp(LD(700))))


def test_served_operands_are_the_logit_of_the_grown_row():
    """c + L_new + fL[j] + A_new . F[j] is the rule's own z for the folded column."""
    case = fc.fold_cases()["special-init-k7"]
    V, w = fc.oracle(case)
    A, L = fc.served_all(case, V, w)
    F, fL = case.fixed()
    g, l = case.feature_sums()
    assert A.shape == (case.n_new, 8) and not A[:, 7].any()
    for r in range(case.n_new):
        for j in range(2, case.n_fixed):
            h = LD(1) * g[r] + F[j]
            z = fc.C0 + LD(l[r]) + fL[j] + (LD(1) * g[r] * F[j]).sum() + w[r] + (V[r] * h).sum()
            got = fc.C0 + L[r] + fL[j] + (A[r, :7] * F[j]).sum()
            assert abs(got - z) <= 1e-17 * 64


# --------------------------------------------------------------------------
# the reference anchor
# --------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["user", "item"])
@pytest.mark.parametrize("k", [3, 12, 130])
def test_one_pass_is_the_reference_step_on_the_grown_model(k, side):
    """One step of cpu_ref.fm_step_closed on the grown model (the new id columns stored last) over the
    batch of ALL examples of several new rows does to the new columns of w and V what one pass does."""
    prob = fc.flow_problem(k, side)
    rng = np.random.default_rng(k)
    w0, w, V = cpu_ref.fm_init(3, prob.n_features, k, alpha=0.3)
    w0[0] = 0.2
    nu0 = rng.uniform(-0.3, 0.3, size=(prob.n_new, k))
    om0 = rng.normal(scale=0.1, size=prob.n_new)
    lr = fc.flow_lr(prob, w, V)
    XU, XI = fc.grown_sides(prob)
    pairs = prob.data["features"].copy()
    col = 0 if side == "user" else 1
    pairs[:, col] += (fc.FLOW_USERS, fc.FLOW_ITEMS)[col]  # the new rows sit behind their side's own
    Xb = fc.pair_rows(XU, XI, pairs[:, 0], pairs[:, 1])
    gw, gV = fc.grown_params(w, V, nu0, om0)
    before = (w0.copy(), gw.copy(), gV.copy())
    cpu_ref.fm_step_closed(Xb, prob.data["labels"], prob.data["pscores"], w0, gw, gV, lr)
    g, l, F, fL = fc.flow_operands(prob, w, V, LD)
    ptr, ids, ry = fc.flow_grouped(prob)
    want_V, want_w = np.zeros((prob.n_new, k), dtype=LD), np.zeros(prob.n_new, dtype=LD)
    for r in range(prob.n_new):
        sl = slice(ptr[r], ptr[r + 1])
        want_V[r], want_w[r] = fc.fold_row(ids[sl], ry[sl], F, fL, g[r], l[r], before[0][0], nu0[r], om0[r], 1, lr)
    worst = fc.assert_within((gV[prob.n_features:], gw[prob.n_features:]), (want_V, want_w), fc.FMFOLD_TOL,
                             f"anchor k{k} {side}", lr)
    print(f"anchor k{k} {side} {worst:.3e}")
    # a row without examples kept its column; the step moved the columns at all
    idle = np.flatnonzero(np.diff(ptr) == 0)
    assert idle.size and (gV[prob.n_features + idle] == nu0[idle]).all()
    assert np.abs(gV[prob.n_features:] - nu0).max() > 1e-4


# --------------------------------------------------------------------------
# mutations: the oracle catches each on the affected row alone
# --------------------------------------------------------------------------
@pytest.mark.parametrize("mutation", ["skips_last", "err_after_omega", "no_g_in_h", "stale_nu"])
def test_oracle_catches_a_mutation_on_its_row_alone(mutation):
    case = fc.fold_cases()["special-k7"]
    want = fc.oracle(case)
    F, fL = case.fixed()
    g, l = case.feature_sums()
    nu0, om0 = case.start()
    ry, ptr = case.ry(), case.row_ptr
    victim = 4  # eleven examples, three passes
    got = [np.asarray(want[0], dtype=np.float64), np.asarray(want[1], dtype=np.float64)]
    sl = slice(ptr[victim], ptr[victim + 1])

    def row(mut):
        return fc.fold_row(case.ids[sl], ry[sl], F, fL, g[victim], l[victim], fc.C0, nu0[victim], om0[victim],
                           case.n_passes, case.lr, mutation=mut)
    got[0][victim], got[1][victim] = row(mutation)
    rows = ms.row_distance(got[0], want[0]).max(axis=1)
    assert rows[victim] > 1e-4, (mutation, float(rows[victim]))  # nine orders above the tolerance
    assert (np.delete(rows, victim) <= fc.FMFOLD_TOL).all()
    with pytest.raises(AssertionError):
        fc.assert_within(got, want, fc.FMFOLD_TOL, mutation, case.lr)
    got[0][victim], got[1][victim] = row(None)
    fc.assert_within(got, want, fc.FMFOLD_TOL, "unmutated", case.lr)


# --------------------------------------------------------------------------
# the flows: rounding cannot reorder a ranking
# --------------------------------------------------------------------------
@pytest.mark.parametrize("side", ["user", "item"])
@pytest.mark.parametrize("k", [12, 13])
def test_flow_logits_are_far_apart(k, side):
    """The smallest gap between adjacent logits of any user of the flows exceeds 1e-9, on the grown
    model with the oracle's folded columns."""
    prob = fc.flow_problem(k, side)
    w0, w, V = fc.flow_fit(prob)
    lr = fc.flow_lr(prob, w, V)
    nu, om = fc.flow_oracle(prob, w0, w, V, lr)
    assert np.abs(np.asarray(nu, dtype=np.float64)).max() > 1e-3  # the fold-in moved the columns
    gw, gV = fc.grown_params(w, V, nu, om)
    XU, XI = fc.grown_sides(prob)
    first = fc.FLOW_USERS if side == "user" else 0  # new users alone / every user over the grown items
    u, i = fc.all_pairs(XU.shape[0], XI.shape[0], first)
    logits = cpu_ref.fm_logit(fc.pair_rows(XU, XI, u, i), w0, gw, gV).reshape(-1, XI.shape[0])
    assert fc.smallest_gap(logits) > 1e-9, fc.smallest_gap(logits)


# --------------------------------------------------------------------------
# grouping, order array and argument checks of the Python entry (no device)
# --------------------------------------------------------------------------
def test_grouping_and_order_are_fold_examples():
    """The host half is fold.fold_examples: grouped by new row with a stable sort, the rows by
    descending example count."""
    from relevance_factorizationmachine_amd.fold import fold_examples
    case = fc.fold_cases()["shape-k7"]
    for side, col in (("user", 0), ("item", 1)):
        for interleaved in (False, True):
            data = case.data(side, interleaved)
            if interleaved:
                assert (np.diff(data["features"][:, col]) < 0).any()  # the input is not grouped
            row_ptr, ids, ry, order = fold_examples(data, case.n_new, case.n_fixed, col, case.n_passes)
            np.testing.assert_array_equal(row_ptr, case.row_ptr)
            np.testing.assert_array_equal(ids, case.ids)
            np.testing.assert_array_equal(ry, case.ry())
            np.testing.assert_array_equal(order, case.order)
    prob = fc.flow_problem(12)
    row_ptr, ids, ry, order = fold_examples(prob.data, prob.n_new, prob.n_fixed, 0, prob.n_passes)
    ptr, want_ids, want_ry = fc.flow_grouped(prob)
    np.testing.assert_array_equal(row_ptr, ptr)
    np.testing.assert_array_equal(ids, want_ids)
    np.testing.assert_array_equal(ry, want_ry)
    assert order.tolist() == [3, 0, 2, 4, 1]


def test_argument_checks_need_no_device():
    from relevance_factorizationmachine_amd import recommend as rec
    from relevance_factorizationmachine_amd.fm import FactorizationMachines, FoldedColumns, fold_rows
    prob = fc.flow_problem(12)
    sides = rec.Sides(prob.XU, prob.XI)
    model = types.SimpleNamespace(n_features=prob.n_features, n_factors=12, lr=0.05, _rt=None)

    def fold(side=0, new_rows=prob.new_rows, data=prob.data, n_passes=1, init=None, model=model, sides=sides, ops=None):
        return FactorizationMachines._fold_in(model, side, sides, new_rows, data, n_passes, init, None, ops)
    X = fold_rows(sides, prob.new_rows, 0, prob.n_features)
    assert X.shape == prob.new_rows.shape and X.has_canonical_format
    with pytest.raises(TypeError, match="Sides"):
        fold(sides=None)
    with pytest.raises(ValueError, match="columns"):
        fold(model=types.SimpleNamespace(n_features=prob.n_features + 1, n_factors=12, lr=0.05, _rt=None))
    with pytest.raises(ValueError, match="new_rows"):
        fold(new_rows=prob.new_rows[:, :-1])
    # a column of the other side: an item's one-hot column in a new user's row, and the converse
    bad = prob.new_rows.tolil()
    bad[0, fc.FLOW_USERS + fc.FLOW_UW + 2] = 1.0
    with pytest.raises(ValueError, match="stored on the item side"):
        fold(new_rows=bad.tocsr())
    with pytest.raises(ValueError, match="stored on the user side"):
        fold(side=1, new_rows=prob.new_rows)
    good = prob.data
    with pytest.raises(IndexError):
        fold(data={**good, "features": np.array([[prob.n_new, 0]]), "labels": np.ones(1), "pscores": np.ones(1)})
    with pytest.raises(IndexError):
        fold(data={**good, "features": np.array([[0, fc.FLOW_ITEMS]]), "labels": np.ones(1), "pscores": np.ones(1)})
    with pytest.raises(IndexError):
        fold(data={**good, "features": np.array([[0, -1]]), "labels": np.ones(1), "pscores": np.ones(1)})
    with pytest.raises(ValueError):
        fold(data={**good, "labels": good["labels"][:-1]})
    with pytest.raises(ValueError):
        fold(data={**good, "pscores": good["pscores"][:-1]})
    with pytest.raises(ValueError):
        fold(n_passes=-1)
    with pytest.raises(ValueError, match="init"):
        fold(init=(np.zeros((prob.n_new, 11)), np.zeros(prob.n_new)))
    with pytest.raises(ValueError, match="init"):
        fold(init=(np.zeros((prob.n_new, 12)), np.zeros(prob.n_new + 1)))
    ops = rec.Operands(None, np.zeros((fc.FLOW_USERS, 12)), None, np.zeros((fc.FLOW_ITEMS + 1, 12)), None, None, 12)
    with pytest.raises(ValueError, match="ops"):
        fold(ops=ops)
    # new_users= of an FM model: the FoldedColumns of fold_in_users and nothing else
    fm = types.SimpleNamespace(n_features=prob.n_features, n_factors=12)
    from relevance_factorizationmachine_amd.mf import FoldedRows
    with pytest.raises(TypeError, match="Sides"):
        rec.operands(fm, sides, new_users=FoldedRows("user", np.zeros((2, 12)), np.zeros(2), None))
    with pytest.raises(TypeError, match="Sides"):
        rec.operands(fm, sides, new_users=FoldedColumns("item", np.zeros(2), np.zeros((2, 12)), np.zeros((2, 12)),
                                                        np.zeros(2), None))
    with pytest.raises(ValueError, match="folded operands"):
        rec.operands(fm, sides, new_users=FoldedColumns("user", np.zeros(2), np.zeros((2, 12)), np.zeros((2, 16)),
                                                        np.zeros(2), None))
    mf = types.SimpleNamespace(n_factors=12, b=0.1)
    with pytest.raises(TypeError):
        rec.operands(mf, new_users=FoldedColumns("user", np.zeros(2), np.zeros((2, 12)), np.zeros((2, 12)), np.zeros(2),
                                                 None))
    with pytest.raises(TypeError):
        FactorizationMachines.append_columns(fm, FoldedRows("user", np.zeros((2, 12)), np.zeros(2), None))
    with pytest.raises(ValueError):
        FactorizationMachines.append_columns(fm, FoldedColumns("user", np.zeros(2), np.zeros((2, 11)), np.zeros((2, 12)),
                                                               np.zeros(2), None))
    folded = FoldedColumns("user", np.zeros(2), np.zeros((2, 12)), np.zeros((2, 12)), np.zeros(2), None)
    assert len(folded) == 2 and folded.side == "user"


# --------------------------------------------------------------------------
# the launch shape the library reports
# --------------------------------------------------------------------------
@pytest.mark.parametrize("cls", list(ms.CLASS_RANGE))
def test_geometry_at_every_class(cls):
    lpr, vec, nc = cls
    for k in ms.CLASS_RANGE[cls]:
        for n_new in (1, fc.ASSUMED_GRID - 1, fc.ASSUMED_GRID + 1, 1 << 22):
            g = fc.geometry(n_new, k)
            assert (g["lpr"], g["vec"], g["nc"]) == cls, (k, g)
            assert g["groups"] == 256 // lpr == fc.groups(k)
            assert g["grid"] == min(n_new, ms.ASSUMED_CUS * fc.GRID_PER_CU)  # one workgroup per new row
            # the partial sums of the lane groups fit the 32 KB the kernel declares
            assert g["groups"] * lpr * vec * nc * 8 <= 32 << 10 and lpr * vec * nc >= fc.pad4(k)
    assert fc.geometry(0, ms.CLASS_RANGE[cls][0])["grid"] == 0


def test_entry_points_reject_bad_arguments():
    from relevance_factorizationmachine_amd import _lib
    lib = _lib.load()
    out = np.zeros(5, dtype=np.int32)
    for n_new, k, ptr in ((1, 0, out.ctypes.data), (1, ms.MAX_FACTORS + 1, out.ctypes.data), (-1, 4, out.ctypes.data),
                          (1, 4, None)):
        assert lib.rfm_fm_fold_geometry(None, n_new, k, ptr) == _lib.RFM_ERR_BAD_ARG
        assert _lib.last_error()
    # without a context nothing is launched: a null ctx is a bad argument like any other null pointer
    one = C.c_void_p(out.ctypes.data)
    assert lib.rfm_fm_fold_in(None, one, one, one, one, 1, one, one, one, one, 1, one, 4, 0.1, 1, one, one, one,
                              one) == _lib.RFM_ERR_BAD_ARG
    assert "ctx" in _lib.last_error()

