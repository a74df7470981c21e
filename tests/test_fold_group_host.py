"""The device grouping of fold-in examples, without a GPU: the NumPy statement of the
device scheme (fold_group_common.py) equals ``fold.fold_examples`` on every case of the list under three
arrival orders of the placements -- so what the kernels are asked to compute is the host's result, and
the result does not depend on the order of the atomics; the workspace and launch shapes at ``ctx == NULL`` against their
restatement; the errors ``group_examples_device`` raises before any device work; and four mistakes, each
caught by the exact comparison on a named case of the list the GPU test runs.

On the code before N18 every test here fails: the entries, the table and the wrappers do not exist."""
import numpy as np
import pytest

import fold_group_common as gc
from relevance_factorizationmachine_amd import _lib, fold


@pytest.fixture(scope="module", autouse=True)
def statement_has_the_librarys_limits():
    """The statement sorts a bin up to ``gc.CAP`` and walks the keys beyond it: the cases built around
    that limit mean what they say only if it is the library's."""
    g = fold.group_geometry(None, gc.CAP + 1, 3)
    assert (g["cap"], g["wave_cap"], g["block"], g["long_block"]) == (gc.CAP, gc.WAVE_CAP, gc.BLOCK, gc.LONG_BLOCK)


@pytest.mark.parametrize("arrival", list(gc.ARRIVALS))
@pytest.mark.parametrize("name", list(gc.group_cases()))
def test_statement_equals_fold_examples(name, arrival):
    case = gc.group_cases()[name]
    got, status = gc.fold_group_np(case.data, case.n_new, case.n_fixed, case.new_col, arrival)
    gc.assert_same(got, gc.want_of(case), f"{name} {arrival}")
    assert status.tolist() == [0, 0, -1, 0]


@pytest.mark.parametrize("arrival", list(gc.ARRIVALS))
@pytest.mark.parametrize("name", list(gc.bad_id_cases()))
def test_statement_leaves_bad_ids_out(name, arrival):
    case = gc.bad_id_cases()[name]
    got, status = gc.fold_group_np(case.data, case.n_new, case.n_fixed, case.new_col, arrival)
    kept = gc.filtered(case.data, case.n_new, case.n_fixed, case.new_col)
    gc.assert_same(got, fold.fold_examples(kept, case.n_new, case.n_fixed, case.new_col, 1), name)
    if name == "bad-both":
        assert status.tolist() == [1, 2, 3, 0]
    else:
        assert status.tolist() == ([3, 0, 0, 0] if case.which == "new" else [0, 3, 0, 0])
    with pytest.raises(IndexError, match="new (user|item) index" if case.which == "new" else "id out of range"):
        fold.fold_examples(case.data, case.n_new, case.n_fixed, case.new_col, 1)


def test_the_cases_reach_every_path():
    cases = gc.group_cases()
    lengths = np.bincount(cases["lognormal"].data["features"][:, 0], minlength=700)
    assert {0, 1, gc.WAVE_CAP, gc.WAVE_CAP + 1, gc.CAP} <= set(lengths.tolist()) and lengths.max() > gc.CAP
    assert 45_000 <= lengths.sum() <= 70_000
    assert (np.diff(cases["lognormal"].data["features"][:, 0]) < 0).any()          # shuffled
    il = cases["lognormal-interleaved"].data["features"][:, 0]
    assert len(set(il[:50].tolist())) == 50                                          # the rows' examples take turns
    for n in (gc.CAP - 1, gc.CAP, gc.CAP + 1):
        assert cases[f"one-row-{n}"].n == n
    # rows of one example each: one bin of CAP + 1 rows in the order pass
    rs = cases["reversed-singles"]
    assert rs.n_new == gc.CAP + 1 and (np.bincount(rs.data["features"][:, 0]) == 1).all()
    e = np.bincount(cases["empty-rows"].data["features"][:, 0], minlength=8)
    assert e[0] == 0 and e[3] == 0 and e[-1] == 0
    g = gc.geometry_py(cases["many-bins"].n, cases["many-bins"].n_new)
    assert cases["many-bins"].n_new > g["bin_grid"] * gc.WAVES
    q = cases["inexact"].data
    exact = (q["labels"] / q["pscores"]) * q["pscores"] == q["labels"]
    assert not exact.all()


def test_the_grouping_source_is_built():
    """The entries' declarations and table: test_host_abi.py; their source is one of the library's."""
    assert "rfm_fold_group.hip" in _lib.SOURCES
    assert all(hasattr(_lib.load(), name) for name in ("rfm_fold_group", "rfm_fold_group_workspace", "rfm_fold_group_geometry"))


SIZES = (0, 1, gc.WAVE_CAP, gc.WAVE_CAP + 1, gc.CAP, gc.CAP + 1, gc.SCAN_TILE - 1, gc.SCAN_TILE, 50_000, 1_020_000,
         2 ** 31 - 1)


def test_workspace_matches_restatement():
    for n in SIZES:
        for n_new in SIZES:
            got = fold.group_workspace(n, n_new)
            assert got == gc.workspace_py(n, n_new) and got % 16 == 0, (n, n_new)
    for n, n_new in ((-1, 1), (1, -1), (2 ** 31, 1), (1, 2 ** 31)):
        with pytest.raises(ValueError, match="out of range"):
            fold.group_workspace(n, n_new)


def test_geometry_matches_restatement():
    for n in SIZES:
        for n_bins in SIZES + (2 ** 31,):
            assert fold.group_geometry(None, n, n_bins) == gc.geometry_py(n, n_bins), (n, n_bins)
    g = fold.group_geometry(None, 1_020_000, 7176)
    assert (g["cap"], g["wave_cap"], g["block"], g["long_block"]) == (gc.CAP, gc.WAVE_CAP, gc.BLOCK, gc.LONG_BLOCK)
    # no launch of a tier no bin can reach
    assert fold.group_geometry(None, gc.WAVE_CAP, 5)["mid_grid"] == 0 and fold.group_geometry(None, gc.CAP, 5)["long_grid"] == 0
    assert fold.group_geometry(None, gc.WAVE_CAP + 1, 5)["mid_grid"] == 1 and fold.group_geometry(None, gc.CAP + 1, 5)["long_grid"] == 1
    for n, n_bins in ((-1, 1), (1, -1), (2 ** 31, 1), (1, 2 ** 31 + 1)):
        with pytest.raises(ValueError, match="out of range"):
            fold.group_geometry(None, n, n_bins)


def test_errors_before_any_device_work():
    """No runtime is passed: whatever reached the device would fail on ``None``."""
    ok = gc.group_cases()["mixed"].data
    for bad in ({**ok, "features": ok["features"][:, 0]}, {**ok, "features": ok["features"][:, :1]}):
        with pytest.raises(ValueError, match=r"\(N, 2\) array"):
            fold.group_examples_device(None, bad, 40, gc.N_FIXED, 0)
    for bad in ({**ok, "labels": ok["labels"][:-1]}, {**ok, "pscores": ok["pscores"][:-1]},
                {**ok, "labels": ok["labels"][:, None]}, {**ok, "pscores": np.float64(0.5)}):
        with pytest.raises(ValueError, match="one of each per example"):
            fold.group_examples_device(None, bad, 40, gc.N_FIXED, 0)
    with pytest.raises(ValueError, match="negative"):
        fold.group_examples_device(None, ok, -1, gc.N_FIXED, 0)
    # the messages are those of fold_examples
    for bad in ({**ok, "features": ok["features"][:, 0]}, {**ok, "labels": ok["labels"][:-1]}):
        with pytest.raises(ValueError) as host:
            fold.fold_examples(bad, 40, gc.N_FIXED, 0, 1)
        with pytest.raises(ValueError) as dev:
            fold.group_examples_device(None, bad, 40, gc.N_FIXED, 0)
        assert str(host.value) == str(dev.value)
    with pytest.raises(ValueError, match="group="):
        fold.group_mode(ok, "gpu")
    assert fold.group_mode(ok, None) == "host" and fold.group_mode(ok, "device") == "device"
    with pytest.raises(ValueError, match="neither may be negative"):
        fold.grouped_examples(None, ok, 40, gc.N_FIXED, 0, -1, "device", True)


@pytest.mark.parametrize("mutation,arrival,name,wrong", [
    ("arrival_order", "reversed", "mixed", {"ids", "ry"}),          # bins left in arrival order
    ("order_ascending", "identity", "mixed", {"order"}),            # order ascending
    ("ties_high", "identity", "equal-counts", {"order"}),           # ties of order towards the higher row
    ("ry_by_position", "identity", "inexact", {"ry"}),              # ry by input position, not by perm
])
def test_each_mistake_is_caught_by_exact_comparison(mutation, arrival, name, wrong):
    case = gc.group_cases()[name]
    want = gc.want_of(case)
    got, _ = gc.fold_group_np(case.data, case.n_new, case.n_fixed, case.new_col, arrival, mutation=mutation)
    assert set(gc.differs(got, want)) == wrong, (mutation, gc.differs(got, want))
    with pytest.raises(AssertionError):
        gc.assert_same(got, want, name)
    sound, _ = gc.fold_group_np(case.data, case.n_new, case.n_fixed, case.new_col, arrival)
    gc.assert_same(sound, want, name)
