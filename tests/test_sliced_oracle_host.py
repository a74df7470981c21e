"""The inputs of test_gpu_sliced_rows.py and the arithmetic of the sliced forward, checked on the CPU
(sliced_rows_common.py): the training logs give the cached columns and the LDS order they are built
for, the class logs hold every class of row they promise -- and every ordered pair of kinds 16 rows
apart inside a workgroup of any size from 41 rows on --, at least 80 % of every log's rows are
unsaturated, a float64 statement of the kernel's sums (in its own and in a shuffled order) stays
below half of forward_rows_common's tol_p on every row of every case, and each of four mutations of
that statement leaves the tolerance on exactly the rows it touches.  No GPU needed."""
import numpy as np
import pytest

import forward_rows_common as fr
import sliced_rows_common as sr

CASES_A = [(64, k) for k in sr.SLICE_TABLE] + [(16, 130), (16, 300), (32, 130), (32, 300)]
# cached-column logs of part B: (frequent columns, factor count)
CASES_B = [(F, 130) for F in (0, 1, 127, 128, 129, 151, 156)] + [(76, 256), (80, 256)]


@pytest.mark.parametrize("k,want", sorted(sr.SLICE_TABLE.items()))
def test_slice_table_is_the_plans_formula(k, want):
    assert sr.slices_of(k) == want
    ns, sw, last = want
    assert sw % 2 == 0 and last % 2 == 0 and 0 < last <= sw <= 256 and (ns - 1) * sw + last == k


def test_lds_cap_of_the_factor_counts_of_part_b():
    assert sr.lds_cap(130) == 151 and sr.lds_cap(256) == 76


@pytest.mark.parametrize("ML", [16, 32, 64])
def test_training_logs_give_the_cached_columns_they_are_built_for(ML):
    log, C, named = sr.train_log(sr.N_FREQ, sr.N_RARE, ML)
    X = log["features"]
    n = X.shape[0]
    assert 1900 <= n <= 2100 and C.F == 64 and C.R >= 70
    cnt = np.bincount(X.indices, minlength=C.n)
    # the plan's rule: at least one row in 64, most frequent first (stable)
    cached = [c for c in range(C.n) if cnt[c] * 64 >= n]
    cached.sort(key=lambda c: -cnt[c])
    np.testing.assert_array_equal(cached, C.freq)
    assert len(set(cnt[C.freq])) == 64 and cnt[C.freq].min() * 16 >= n and cnt[C.rare].max() * 256 <= n
    assert np.diff(X.indptr).max() == ML and sr.records_per_row(ML) == ML
    # interleaved in index: between two neighbouring frequent columns lies a rare one
    f = np.sort(C.freq)
    assert (np.diff(f) > 1).all() and f[0] > 0
    assert all((np.diff(X.indices[X.indptr[r]: X.indptr[r + 1]]) > 0).all() for r in range(n))


@pytest.mark.parametrize("F,k", CASES_B)
def test_cached_column_logs_of_part_b(F, k):
    log, C, _ = sr.train_log(F, sr.EDGE_RARE, 64)
    X = log["features"]
    cnt = np.bincount(X.indices, minlength=C.n)
    cached = sorted((c for c in range(C.n) if cnt[c] * 64 >= X.shape[0]), key=lambda c: -cnt[c])
    np.testing.assert_array_equal(cached, C.freq)
    assert len(C.freq) == F and np.diff(X.indptr).max() == 64
    # the rows scored on it: the marked columns exist where they should, the statement holds
    H = min(F, sr.lds_cap(sr.slices_of(k)[1]))
    ev, marked = sr.edge_log(F, H)
    assert set(marked) == ({"first", "last"} if F else set()) | ({"rank 128"} if H > 128 else set()) | (
        {"cut"} if F > H else set())
    theta = sr.theta(k, C.n)
    o = fr.row_oracle(ev["features"], *theta)
    assert fr.unsaturated_share(o) >= 0.8 and o.length[0] == 0 and o.length[-1] == 0
    assert o.length.max() == F + 5
    got = sr.kernel_statement(ev["features"], *theta, C.freq[:H], k)
    fr.assert_scores(got, o, k, "float64 statement", bound=0.5)


@pytest.mark.parametrize("ML", [16, 32, 64])
def test_class_log_holds_every_class(ML):
    log, nh, ng = sr.class_log(ML)
    X = log["features"]
    n = X.shape[0]
    assert 300 <= n <= 500
    C = sr.Columns(sr.N_FREQ, sr.N_RARE)
    hot = np.isin(X.indices, C.freq)
    row = np.repeat(np.arange(n), np.diff(X.indptr))
    np.testing.assert_array_equal(np.bincount(row[hot], minlength=n), nh)
    np.testing.assert_array_equal(np.bincount(row[~hot], minlength=n), ng)
    have = list(zip(nh.tolist(), ng.tolist()))
    for h in sr.NH_GRID:
        for g in sr.NG_GRID:
            assert have.count((h, g)) >= 2, (h, g)
    for spec in ((ML, 0), (0, ML), (ML - 1, 1), (ML - 3, 3)):
        assert have.count(spec) >= 2, spec
    L = nh + ng
    for length in (ML + 1, 65, 128, 129):
        rows = L == length
        assert (rows & (nh > 0) & (ng > 0)).sum() >= 2 and (rows & (nh == 0)).sum() >= 2, length
        assert ((rows & (ng == 0)).sum() >= 2) == (length <= sr.N_FREQ), length
    assert L[0] == 0 and L[-1] == 0 and (L == 0).sum() >= 6
    # a sorted mixed row alternates between the kinds somewhere: the translation has to reorder it
    mixed = np.flatnonzero((nh >= 2) & (ng >= 2) & (L <= ML))
    assert any((np.diff(hot[X.indptr[r]: X.indptr[r + 1]].astype(int)) != 0).sum() >= 3 for r in mixed)
    # every ordered pair of kinds 16 rows apart inside one workgroup, whatever its size from 41 rows on
    masks = sr.kind_masks(nh, ng, ML)
    for rpw in range(41, n + 1):
        inside = sr.pairs_inside(masks, rpw)
        assert inside.all(), (rpw, [(sr.KINDS[a], sr.KINDS[b]) for a, b in zip(*np.nonzero(~inside))])


@pytest.mark.parametrize("ML,k", CASES_A)
def test_float64_statement_stays_below_half_of_the_tolerance(ML, k):
    log, nh, ng, theta, o = sr.class_case(ML, k)
    assert fr.unsaturated_share(o) >= 0.8 and np.isfinite(o.p).all(), fr.unsaturated_share(o)
    np.testing.assert_array_equal(o.length, nh + ng)
    C = sr.Columns(sr.N_FREQ, sr.N_RARE)
    for shuffled in (False, True):
        got = sr.kernel_statement(log["features"], *theta, C.freq, k, shuffled=shuffled, seed=k)
        fr.assert_scores(got, o, k, f"float64 statement, shuffled={shuffled}", bound=0.5)


@pytest.mark.parametrize("k", [300, 514])
def test_tiled_base_log_and_training_logs_are_unsaturated(k):
    """The other logs the device tests score: the 1 021-row base of the tiled launch, the training log
    of part D with its long and empty rows, the logs of part B."""
    log, nh, ng, theta, o = sr.class_case(64, k, 1021 - sr.class_log(64)[0]["features"].shape[0])
    assert log["features"].shape[0] == 1021 and fr.unsaturated_share(o) >= 0.8
    tlog, C, named = sr.train_log(sr.N_FREQ, sr.N_RARE, 64, (65, 130), 3)
    to = fr.row_oracle(tlog["features"], *sr.theta(k, C.n))
    assert fr.unsaturated_share(to) >= 0.8
    assert [int(to.length[r]) for r in named["long"]] == [65, 130] and (to.length[named["empty"]] == 0).all()
    got = sr.kernel_statement(tlog["features"][:200], *sr.theta(k, C.n), C.freq, k)
    fr.assert_scores(got, to.take(slice(0, 200)), k, "training rows", bound=0.5)


@pytest.mark.parametrize("ML,k", [(64, 514), (16, 300)])
def test_mutations_leave_the_tolerance_on_exactly_the_affected_rows(ML, k):
    log, nh, ng, theta, o = sr.class_case(ML, k)
    C = sr.Columns(sr.N_FREQ, sr.N_RARE)
    affected = {1: nh >= 5, 2: ng >= 3, 3: nh + ng >= 2, 4: nh >= 1}
    for mutation, rows in affected.items():
        assert 10 < rows.sum() < len(rows)
        got = sr.kernel_statement(log["features"], *theta, C.freq, k, mutation=mutation)
        ex = fr.score_excess(got, o, k)
        np.testing.assert_array_equal(~(ex <= 1.0), rows, err_msg=f"mutation {mutation}")
        assert (ex[~rows] <= 0.5).all()
