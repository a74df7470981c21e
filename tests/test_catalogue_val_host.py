"""Host half of the per-iteration catalogue metrics: what
``evaluate.CatalogueValEvaluator`` checks and prepares before any device call, and the new
symbols of the library.  No GPU needed."""
import types

import numpy as np
import pytest
from scipy import sparse as sp

import rank_items_common as rk
from relevance_factorizationmachine_amd import _lib, evaluate
from relevance_factorizationmachine_amd.evaluate import CatalogueValEvaluator

NI = 7
POS = (np.array([0, 0, 2, 3]), np.array([1, 4, 6, 0]))


def _make(positives=POS, n_items=NI, K=(1, 3), used=("DCG", "MRR"), monitor=("DCG", 3), **kw):
    return CatalogueValEvaluator(positives, n_items, list(K), list(used), monitor, **kw)


def test_constructor_keeps_what_it_was_given():
    ev = _make(every=4)
    assert ev.K == [1, 3] and ev.used_metrics == ["DCG", "MRR"] and ev.monitor == ("DCG", 3) and ev.every == 4
    assert ev.n_columns == 8 and ev.unranked == 0 and ev.history == {} and ev.unranked_history.shape == (0,)
    np.testing.assert_array_equal(ev._sel, [0, 2, 3])
    np.testing.assert_array_equal(ev._indptr, [0, 2, 3, 4])
    assert ev._sel.dtype == np.int32 and ev._indptr.dtype == np.int64


@pytest.mark.parametrize("monitor", [("Recall", 3), ("DCG", 5), ("DCG", None), ("MRR", 3), ("nDCG", 1), "DCG", ("DCG",),
                                     ("DCG", 3.0), ("DCG", True)])
def test_bad_monitor(monitor):
    with pytest.raises(ValueError, match="monitor"):
        _make(monitor=monitor)


def test_monitor_without_a_depth():
    assert _make(used=("MRR", "AUC"), monitor=("AUC", None))._monitor == ("AUC", 0)
    assert _make(used=("MRR", "AUC"), monitor=("MRR", None))._monitor == ("MRR", 0)
    assert _make(K=(5, 1, 3), monitor=("DCG", 3))._monitor == ("DCG", 2)


@pytest.mark.parametrize("every", [0, -1, 1.5, None, True])
def test_every_must_be_a_positive_integer(every):
    with pytest.raises(ValueError, match="every"):
        _make(every=every)


def test_pscores_are_checked():
    for bad in (np.ones(3), np.ones((4, 1)), [1.0, 0.0, 1.0, 1.0], [1.0, -0.5, 1.0, 1.0], [1.0, np.nan, 1.0, 1.0],
                [1.0, np.inf, 1.0, 1.0]):
        with pytest.raises(ValueError, match="pscores"):
            _make(pscores=bad)
    # a pair given twice: the same propensity is fine, two different ones are not
    twice = (np.array([0, 2, 0]), np.array([1, 6, 1]))
    ev = _make(positives=twice, pscores=[0.5, 0.25, 0.5])
    np.testing.assert_array_equal(ev.pscores, [0.5, 0.25])
    with pytest.raises(ValueError, match="two different pscores"):
        _make(positives=twice, pscores=[0.5, 0.25, 0.4])


def test_repeats_are_dropped_and_the_targets_grouped():
    users, items = np.array([3, 0, 3, 0, 0, 3]), np.array([5, 2, 5, 1, 2, 0])
    ev = _make(positives=(users, items), pscores=[0.9, 0.2, 0.9, 0.1, 0.2, 0.3])
    np.testing.assert_array_equal(ev.users, [0, 0, 3, 3])
    np.testing.assert_array_equal(ev.items, [1, 2, 0, 5])
    np.testing.assert_array_equal(ev.pscores, [0.1, 0.2, 0.3, 0.9])  # follow their pairs
    np.testing.assert_array_equal(ev._sel, [0, 3])
    np.testing.assert_array_equal(ev._indptr, [0, 2, 4])
    base = evaluate.CatalogueEvaluator((users, items), NI, [1, 3], ["DCG", "MRR"])
    np.testing.assert_array_equal(ev.users, base.users)
    np.testing.assert_array_equal(ev.items, base.items)


def test_the_checks_of_the_catalogue_evaluator_hold():
    with pytest.raises(ValueError, match="outside"):
        _make(positives=(np.array([0]), np.array([NI])))
    with pytest.raises(ValueError, match="outside"):
        _make(positives=(np.array([0]), np.array([-1])))
    with pytest.raises(ValueError, match="negative"):
        _make(positives=(np.array([-1]), np.array([0])))
    with pytest.raises(ValueError, match="integer"):
        _make(positives=(np.array([0.0]), np.array([1.0])))
    with pytest.raises(ValueError, match="equal length"):
        _make(positives=(np.array([0, 1]), np.array([1])))
    with pytest.raises(ValueError, match="positive integers"):
        _make(K=(0, 3))
    with pytest.raises(ValueError, match="unknown metric"):
        _make(used=("DCG", "Gini"))
    with pytest.raises(ValueError, match="1 to 16 depths"):
        _make(K=range(1, 18), monitor=("DCG", 1))
    with pytest.raises(ValueError, match="1 to 16 depths"):
        _make(K=(), used=("MRR",), monitor=("MRR", None))
    with pytest.raises(ValueError, match="sides"):
        _make(sides=object())


def test_an_excluded_positive_is_refused_at_construction():
    E = sp.csr_matrix((np.ones(3), (np.array([0, 1, 3]), np.array([2, 1, 0]))), shape=(4, NI))
    with pytest.raises(ValueError, match="exclusion list"):
        _make(exclude=E)  # (3, 0) is a positive
    with pytest.raises(ValueError, match="exclusion list"):
        _make(exclude=(E.indptr, E.indices))
    ok = sp.csr_matrix((np.ones(2), (np.array([0, 1]), np.array([2, 1]))), shape=(4, NI))
    ev = _make(exclude=ok)
    np.testing.assert_array_equal(ev._excl[0], [0, 1, 2, 2, 2])
    with pytest.raises(ValueError, match="exclude"):
        _make(exclude=sp.csr_matrix((4, NI + 1)))


def _stub(kind):
    if kind == "fm":
        return types.SimpleNamespace(n_features=12, n_factors=4, estimator="IPS")
    return types.SimpleNamespace(n_users=4, n_items=NI, n_factors=4, estimator="IPS", b=0.5)


def test_sides_must_fit_the_kind_of_model():
    """Raised before anything touches a device: a stand-in with the model's shape fields is enough."""
    from relevance_factorizationmachine_amd.recommend import Sides

    with pytest.raises(ValueError, match="needs sides"):
        _make().evaluate(_stub("fm"))
    with pytest.raises(ValueError, match="needs sides"):
        _make().fit_begin(_stub("fm"), 3)
    XU = sp.csr_matrix(np.hstack([np.eye(4), np.zeros((4, NI))]))
    XI = sp.csr_matrix(np.hstack([np.zeros((NI, 4)), np.eye(NI)]))
    sides = Sides(XU, XI)
    with pytest.raises(ValueError, match="takes no sides"):
        _make(sides=sides).evaluate(_stub("mf"))
    with pytest.raises(ValueError, match="takes no sides"):
        _make(sides=sides).fit_begin(_stub("mf"), 3)
    with pytest.raises(ValueError, match="columns"):
        _make(sides=sides).evaluate(_stub("fm"))  # 11 columns against the model's 12
    with pytest.raises(ValueError, match="n_items"):
        _make(n_items=NI + 1).evaluate(_stub("mf"))
    with pytest.raises(ValueError, match="user id"):
        _make(positives=(np.array([4]), np.array([0]))).evaluate(_stub("mf"))
    with pytest.raises(ValueError, match="exclude lists"):
        _make(exclude=sp.csr_matrix((5, NI))).evaluate(_stub("mf"))


def test_when_the_evaluation_is_due():
    ev = _make(every=3)
    ev._fit = {"n_epochs": 8}
    assert [e for e in range(8) if ev.fit_due(e)] == [2, 5, 7]
    assert [ev.fit_run_length(e) for e in range(8)] == [3, 2, 1, 3, 2, 1, 2, 1]
    ev = _make(every=1)
    ev._fit = {"n_epochs": 4}
    assert all(ev.fit_due(e) for e in range(4)) and [ev.fit_run_length(e) for e in range(4)] == [1] * 4
    ev = _make(every=10)
    ev._fit = {"n_epochs": 4}
    assert [e for e in range(4) if ev.fit_due(e)] == [3] and ev.fit_run_length(0) == 4


def test_result_rows_are_split_by_metric():
    ev = _make(K=(1, 3), used=("AUC", "MAP", "DCG"), monitor=("MAP", 1))
    out = ev._split(np.arange(16, dtype=np.float64).reshape(2, 8))
    assert list(out) == ["AUC", "MAP", "DCG"]
    np.testing.assert_array_equal(out["DCG"], [[0, 1], [8, 9]])
    np.testing.assert_array_equal(out["MAP"], [[4, 5], [12, 13]])
    np.testing.assert_array_equal(out["AUC"], [[7], [15]])


def test_it_is_not_taken_for_the_reference_evaluator():
    ev = _make()
    assert evaluate.known_implementation(ev) is False
    assert evaluate.recognise(ev, "IPS") is None and evaluate.recognise(ev, "Naive") is None
    assert evaluate.recognise(ev, "IPS", any_implementation=True) is None
    assert evaluate.host_frame(ev, "IPS", 4) is None


def test_fit_data_parallel_refuses_it_before_any_work():
    from relevance_factorizationmachine_amd import dist

    model = types.SimpleNamespace(evaluator=_make(), n_epochs=3)
    with pytest.raises(NotImplementedError, match="CatalogueValEvaluator"):
        dist.fit_data_parallel(model, {}, {})


def test_library_exports_the_new_symbols():
    import ctypes as C

    lib = _lib.load()
    for name in ("rfm_pair_ranks_n", "rfm_rank_metrics", "rfm_rank_metrics_workspace", "rfm_fm_train_part"):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["rfm_pair_ranks_n"]) == len(_lib.SIGNATURES["rfm_pair_ranks"]) + 1
    out = C.c_int64(0)
    _lib.check(lib.rfm_rank_metrics_workspace(10, 100, 5, C.byref(out)))
    assert out.value == 10 * 17 * 8 + 100 * 8 + 10 * 4  # per-user rows, ordered ranks + sources, unranked counts
    _lib.check(lib.rfm_rank_metrics_workspace(0, 0, 1, C.byref(out)))
    assert out.value >= 16
    for n_K in (0, 17):
        with pytest.raises(ValueError, match="n_K"):
            _lib.check(lib.rfm_rank_metrics_workspace(10, 100, n_K, C.byref(out)))
    assert set(rk.METRICS) == set(CatalogueValEvaluator.METRICS)
