"""What test_gpu_plan_history.py runs, checked without a GPU: the sequences of calls cover every
hand-over between two entry points, every change of forward shape around each of them and, for
the factor counts of two slot bitmaps, both parities of the step counter; the id generators give
what their names say; the logs have the row lengths and column classes the GPU tests count on;
the gradient oracle on CSR entries is the dense long-double statement of grad_forms_common."""
import numpy as np
import pytest

import grad_forms_common as gf
import plan_history_common as ph

CLASSES = sorted(ph.SEQUENCES)


def _sizes(name):
    k, _, full = ph.CASES[name]
    sizes = ph.host_sizes(k, capped=ph.K400_MAX_BATCH if full == "max" else None)
    return sizes, sizes[full] + ph.EXTRA_ROWS


def test_every_sequence_belongs_to_a_case_and_fits():
    assert sorted(ph.SEQUENCE_OF) == sorted(ph.CASES)
    for name, seq in ph.SEQUENCE_OF.items():
        sizes, _ = _sizes(name)
        assert 0 < len(seq) <= ph.MAX_CALLS, (name, len(seq))
        for c in seq:
            assert c.entry in ph.ENTRIES and c.ids in ph.IDS_KINDS + ("-",), c
            assert c.shape == ph.UNSHAPED[c.entry] if c.entry in ph.UNSHAPED else c.shape in sizes, (name, c)


@pytest.mark.parametrize("k_class", CLASSES)
def test_every_ordered_pair_of_entries_is_adjacent_somewhere(k_class):
    pairs, _, _, _ = ph.coverage(list(ph.SEQUENCES[k_class].values()))
    assert not ph.ALL_PAIRS - pairs, sorted(ph.ALL_PAIRS - pairs)


@pytest.mark.parametrize("k_class", CLASSES)
def test_every_change_of_shape_class_occurs_around_every_entry(k_class):
    _, around, _, _ = ph.coverage(list(ph.SEQUENCES[k_class].values()))
    assert not ph.ALL_AROUND - around, sorted(ph.ALL_AROUND - around)


def test_shape_classes_are_the_two_forward_shapes():
    """one, group, below (mid) take the one-row shape, min, min+1, trip2 (max) the many-rows shape:
    on the sizes forward_form gives a device of 256 compute units."""
    for name in ph.CASES:
        sizes, _ = _sizes(name)
        m = sizes.get("min", sizes.get("mid", 0) + 1)
        for shape, rows in sizes.items():
            assert ph.SHAPE_CLASS[shape] == ("large" if rows >= m else "small"), (name, shape, rows, m)


def test_both_parities_of_the_step_counter_before_the_same_call():
    """Chunked factor counts: per entry that advances the counter, some (entry, shape) is called
    after an even and after an odd number of increments."""
    _, _, _, parity = ph.coverage(list(ph.SEQUENCES["chunked"].values()))
    for entry in ph.ENTRIES:
        if ph.ADVANCE[entry]:
            assert any(e == entry and p == {0, 1} for (e, _), p in parity.items()), entry
    for name, seq in ph.SEQUENCES["chunked"].items():  # ... and in each of the two sequences: a step
        _, _, _, par = ph.coverage([seq])
        assert any(e == "step" and p == {0, 1} for (e, _), p in par.items()), name


@pytest.mark.parametrize("k_class", CLASSES)
def test_every_ids_kind_follows_a_full_batch(k_class):
    _, _, after_full, _ = ph.coverage(list(ph.SEQUENCES[k_class].values()))
    assert {"same", "disjoint", "overlap"} <= after_full, after_full


@pytest.mark.parametrize("name", sorted(ph.CASES))
def test_ids_are_what_their_kind_says(name):
    sizes, n_rows = _sizes(name)
    seq = ph.SEQUENCE_OF[name]
    prev = None
    for c, ids in zip(seq, ph.resolve(seq, sizes, n_rows, 0)):
        if ids is None:
            assert c.entry in ph.UNSHAPED
            continue
        its = ids if ids.ndim == 2 else ids[None, :]
        assert its.shape == (ph.increments(c) if ids.ndim == 2 else 1, sizes[c.shape]) and its.dtype == np.int32
        for b in its:
            assert len(np.unique(b)) == len(b) and b.min() >= 0 and b.max() < n_rows, c
        if prev is not None and c.ids == "same":
            np.testing.assert_array_equal(its[0], prev)
        if prev is not None and c.ids == "disjoint":
            assert not np.intersect1d(its[0], prev).size, c
        if prev is not None and c.ids == "overlap":
            shared = np.intersect1d(its[0], prev).size
            assert shared >= 1 and (shared < len(its[0]) or len(its[0]) == 1 or len(prev) + len(its[0]) > n_rows), c
        prev = its[-1]


@pytest.mark.parametrize("n_rows,seed", [(4397, 0), (ph.VAL_SMALL, 1), (ph.VAL_BIG, 2)])
def test_logs(n_rows, seed):
    log = ph.history_log(n_rows, seed)
    X = log["features"]
    lens = np.diff(X.indptr)
    assert X.shape == (n_rows, ph.N_COLS) and lens.max() == 16 and X.has_sorted_indices
    for L in ph.EDGES:
        assert (lens == L).sum() >= n_rows // 20, (L, int((lens == L).sum()))
    for r in range(n_rows):
        assert len(np.unique(X.indices[X.indptr[r]: X.indptr[r + 1]])) == lens[r]
    cnt = np.bincount(X.indices, minlength=ph.N_COLS)
    assert cnt[0] == (lens >= 1).sum() and cnt[1] == (lens >= 2).sum()  # two columns in every row that has room
    if n_rows > 4000:
        assert ph.hot_mode_for(log, n_rows - ph.EXTRA_ROWS) > cnt[ph.N_FREQ:].max()
        assert np.count_nonzero(cnt[: ph.N_FREQ] > 256) >= 2  # longer than a workgroup's slots at 64 lanes per row
        few = np.unique(X[:17].indices)
        assert len(few) < ph.N_COLS // 10  # a small batch touches a few columns only
    other = ph.history_log(n_rows, seed, 1)  # other contents in the same arrays: the same row lengths
    np.testing.assert_array_equal(other["features"].indptr, X.indptr)
    assert not np.array_equal(other["features"].indices, X.indices) and not np.array_equal(other["features"].data, X.data)


@pytest.mark.parametrize("k", [20, 65])
def test_entry_oracle_is_the_dense_oracle(k):
    """Both are long-double sums of the same terms in different orders: they differ by rounding,
    far below the 1e-11 * S the device is held to."""
    log = ph.history_log(900, 3)
    ids = np.random.default_rng(k).permutation(900)[:700].astype(np.int32)
    th = ph.theta(k)
    got, want = ph.grad_oracle(log, ids, *th), gf.grad_oracle(log, ids, *th)
    for g, w, S, name in zip(got[:3], want[:3], want[3], ("g_w0", "g_w", "G_V")):
        assert np.shape(g) == np.shape(w)
        assert np.all(np.abs(g - w) <= 1e-16 * np.asarray(S)), name
    for a, b in zip(got[3], want[3]):
        assert np.all(np.abs(a - b) <= 1e-16 * np.abs(b))
    assert np.count_nonzero(want[3][1]) > ph.N_FREQ  # (the batch holds sparse columns too)
