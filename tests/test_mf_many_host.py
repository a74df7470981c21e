"""Several MF models on one schedule, without a GPU: the shared host scheduler (rfm_mf_schedule_rows)
against rfm_mf_schedule_ex on every case of mf_step_common.py, the launch shapes of the many-model
calls (rfm_mf_many_geometry) against a Python restatement, and a float64 statement of "M models on one
schedule" that stays at the floor of the long-double oracle while each of the three mistakes the new
kernels can make -- a neighbour's label / propensity, a cache written back into another model, the
record-to-row indirection dropped -- exceeds ``MF_TOL`` on the affected models alone.  So the GPU
test's cases and tolerance see exactly those errors."""
import numpy as np
import pytest

import mf_many_common as mm
import mf_step_common as ms
from relevance_factorizationmachine_amd import _lib
from relevance_factorizationmachine_amd.runtime import mf_many_geometry, mf_schedule, mf_schedule_ex, mf_schedule_rows


def test_many_model_structs_and_limit_are_the_headers():
    """The two structs of a many-model call have the sizes include/rfm_hip.h states, and the model limit is its
    ``RFM_MF_MAX_MODELS`` (the declarations themselves: test_host_abi.py)."""
    import ctypes as C
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "rfm_hip.h")).read()
    assert C.sizeof(_lib.MfModel) == 64 and C.sizeof(_lib.MfLabels) == 16
    assert int(re.search(r"#define RFM_MF_MAX_MODELS (\d+)", header).group(1)) == _lib.MF_MAX_MODELS


@pytest.mark.parametrize("name", list(ms.step_cases()))
def test_schedule_rows_is_schedule_ex_with_rows(name):
    case = ms.step_cases()[name]
    rows = mm.log_rows(case)
    assert not np.array_equal(rows, np.arange(len(rows))) or len(rows) < 2
    y, p = case.ry()
    cap = ms.capacity(case.k) if case.cache_cap is None else case.cache_cap
    ex0, lptr0, cache0 = mf_schedule_ex(case.users, case.items, y, p, case.n_users, case.n_items, cap)
    ex, ex_rows, lptr, cache = mf_schedule_rows(case.users, case.items, rows, case.n_users, case.n_items, cap)
    for f in ("u", "i", "cslot", "gap"):
        np.testing.assert_array_equal(ex[f], ex0[f], err_msg=f)
    np.testing.assert_array_equal(lptr, lptr0)
    np.testing.assert_array_equal(cache, cache0)
    assert np.isnan(ex["ry"]).all() and len(ex) == len(case.users)
    order, _ = mf_schedule(case.users, case.items, case.n_users, case.n_items)
    np.testing.assert_array_equal(ex_rows, rows[order])
    # the per-thread scratch is reset: a second call gives the same answer
    again = mf_schedule_rows(case.users, case.items, rows, case.n_users, case.n_items, cap)
    for a, b in zip((ex_rows, lptr, cache), again[1:]):
        np.testing.assert_array_equal(a, b)


def test_schedule_rows_edges():
    z = np.zeros(0, np.int32)
    ex, ex_rows, lptr, cache = mf_schedule_rows(z, z, z, 4, 4, 3)
    assert len(ex) == 0 and len(ex_rows) == 0 and lptr.tolist() == [0] and len(cache) == 0
    with pytest.raises(ValueError):
        mf_schedule_rows(np.array([5]), np.array([0]), np.array([0]), 4, 4, 3)
    with pytest.raises(ValueError):
        mf_schedule_rows(np.array([1, 2]), np.array([0, 1]), np.array([0]), 4, 4, 3)


@pytest.mark.parametrize("k", [lo for lo, _ in ms.CLASS_RANGE.values()] + [300, 400, 1024])
def test_geometry_matches_restatement(k):
    per_wg = ms.MF_BLOCK // ms.shape_class(k)[0]
    for n_models in (1, 3, ms.ASSUMED_CUS + 1, 1024):
        for n_recs in (0, 1, per_wg, per_wg + 1, ms.grid_pass(k, ms.ASSUMED_CUS), ms.grid_pass(k, ms.ASSUMED_CUS) + 37):
            assert mf_many_geometry(None, n_models, k, n_recs) == mm.geometry_py(n_models, k, n_recs), (n_models, n_recs)


def test_geometry_rejects_model_counts_out_of_range():
    assert _lib.MF_MAX_MODELS == 1024
    for n_models in (0, 1025, -1):
        with pytest.raises(ValueError, match="n_models"):
            mf_many_geometry(None, n_models, 16, 10)
    with pytest.raises(ValueError):
        mf_many_geometry(None, 1, 0, 10)


STATEMENT_CASES = ("shape-k2", "shape-k16", "ring-cached-k16", "ring-full-k300", "limit-cache-k400", "limit-grow-k300")


@pytest.fixture(scope="module")
def stated():
    """case name -> (case, schedule, models, their oracles): computed once."""
    out = {}
    for name in STATEMENT_CASES:
        case = ms.step_cases()[name]
        models = mm.models_of(case, 3)
        out[name] = (case, mm.reach_rows(case), models, [mm.oracle_of(case, mod) for mod in models])
    return out


@pytest.mark.parametrize("name", STATEMENT_CASES)
def test_statement_stays_at_the_floor(stated, name):
    case, sched, models, want = stated[name]
    got = mm.many_models_f64(case, sched, models)
    for mod, g, w in zip(models, got, want):
        d = ms.assert_params_within(g, w, mod.init, case.pairs, ms.MF_FLOOR, f"{name} model {mod.m}")
        print(f"floor {name} model {mod.m} {d:.3e}")


@pytest.mark.parametrize("mutation,affected", [("neighbour_ry", {1}), ("cache_to_model0", {0}),
                                               ("rows_unpermuted", {0, 1, 2})])
@pytest.mark.parametrize("name", STATEMENT_CASES)
def test_each_mistake_exceeds_the_tolerance_on_the_affected_models_alone(stated, name, mutation, affected):
    case, sched, models, want = stated[name]
    got = mm.many_models_f64(case, sched, models, mutation)
    for mod, g, w in zip(models, got, want):
        d = mm.distance(g, w)
        if mod.m in affected:
            assert d > ms.MF_TOL, (name, mutation, mod.m, d)
        else:
            assert d <= ms.MF_FLOOR, (name, mutation, mod.m, d)
