"""The exact MF batch step -- rfm_mf_sgd_levels_ex, rfm_mf_sgd_levels, rfm_mf_sgd_hogwild on disjoint
rows, rfm_mf_predict, rfm_mf_predict_loss -- through the raw C ABI against the long-double oracle of
mf_step_common.py: at every (lanes per row, vector width, chunks per lane) class of the kernels, on
both sides of the read-ahead boundary, at the launch limits of the sequential kernel, in every state
of its item cache, and past one pass of the capped grids.  Needs an MI355X: ``pytest -m gpu``.

Every case first asserts, from the library's own host scheduler, that it reaches the launches and the
record states it is named for (``mf_step_common.reach``; test_mf_oracle_host.py does the same without
a GPU).  Every call is made twice from the same start and must give the same bits: the exact path has
no floating-point atomics.  P and Q are held to the oracle element by element relative to their own
row, biases relative to max(|b|, lr), at ``MF_TOL`` (derived from a CPU measurement, see that
module); rows of users and items outside the batch, and the sentinels around every array, keep
their bits."""
import numpy as np
import pytest

import mf_step_common as ms
from conftest import rel_err
from oracle import cpu_ref

pytestmark = pytest.mark.gpu

TIGHT = 1e-9  # the norm-wise bound of the parity tests (test_gpu_parity.py), for the fits of e.


@pytest.fixture(scope="module")
def rt():
    from relevance_factorizationmachine_amd import runtime
    return runtime.Runtime.get()


def _n_cu(rt):
    import torch
    return int(torch.cuda.get_device_properties(rt.device).multi_processor_count)


def _twice(run):
    first, second = run(), run()
    for a, b in zip(first, second):
        np.testing.assert_array_equal(a, b, err_msg="two calls from the same start differ")
    return first


def _check(rt, case, entries, want=None):
    sched = ms.reach(case)  # asserts the launches and record states the case is named for
    init = case.init()
    want = ms.oracle(case) if want is None else want
    runs = {"levels_ex": lambda: ms.run_levels_ex(rt, case, sched, init),
            "levels": lambda: ms.run_levels(rt, case, init),
            "hogwild": lambda: ms.run_hogwild(rt, case, init)}
    out = {}
    for entry in entries:
        got = out[entry] = _twice(runs[entry])
        d = ms.assert_params_within(got, want, init, case.pairs, ms.MF_TOL, f"{case.name} {entry}")
        print(f"distance {case.name} {entry} {d:.3e}")
        # the ring's unused loads read row 0 of each array
        for absent, idx in ((not (case.users == 0).any(), (0, 2)), (not (case.items == 0).any(), (1, 3))):
            for j in idx if absent else ():
                np.testing.assert_array_equal(got[j][0], init[j][0], err_msg=f"{case.name} {entry}: row 0 changed")
    return out


def _names(prefix):
    return [n for n in ms.step_cases() if n.startswith(prefix)]


# --------------------------------------------------------------------------
# a. every shape class, at its lowest and highest factor count, both entry points
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("shape-"))
def test_every_shape_class(rt, name):
    case = ms.step_cases()[name]
    assert [p[0] for p in case.want_plan["levels_ex"]] == [p[0] for p in case.want_plan["levels"]] == ["wide", "seq"]
    got = _check(rt, case, ("levels_ex", "levels"))
    # the two forms run the same mf_update on the same values in the same order, and label / propensity
    # is the same IEEE division on the host (the records) and on the device (the plain form)
    for name_, a, b in zip(("P", "Q", "b_u", "b_i"), got["levels"], got["levels_ex"]):
        np.testing.assert_array_equal(a, b, err_msg=f"{case.name}: {name_} of levels and levels_ex differ")


# --------------------------------------------------------------------------
# b. the read-ahead ring: user periods 1..6, the three item kinds, a full workgroup, the start slots
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("ring-"))
def test_read_ahead_ring(rt, name):
    _check(rt, ms.step_cases()[name], ("levels_ex",))


# --------------------------------------------------------------------------
# c. the launch limits and the item cache
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", _names("limit-"))
def test_launch_limits(rt, name):
    _check(rt, ms.step_cases()[name], ("levels_ex",))


# --------------------------------------------------------------------------
# d. more work than one pass of the capped grid
# --------------------------------------------------------------------------
_GRID = {}


def _grid(rt, k):
    if k not in _GRID:
        case = ms.grid_case(k, _n_cu(rt))
        _GRID[k] = (case, ms.oracle_of(case))
    return _GRID[k]


@pytest.mark.parametrize("entry", ["levels_ex", "hogwild"])
@pytest.mark.parametrize("k", ms.GRID_KS)
def test_grid_stride_sgd(rt, k, entry):
    """pass + 37 disjoint examples: one wide level for rfm_mf_sgd_levels_ex; rfm_mf_sgd_hogwild is
    exact on them because no row is shared."""
    case, want = _grid(rt, k)
    assert len(case.users) > ms.grid_pass(k, _n_cu(rt))
    _check(rt, case, (entry,), want)


@pytest.mark.parametrize("k", [lo for lo, _ in ms.CLASS_RANGE.values()])
def test_predict_every_class(rt, k):
    """rfm_mf_predict / rfm_mf_predict_loss: with and without row_ids, 1 / one short of a workgroup /
    one over / (k = 128, 2) more than one pass of the grid rows, out_pred = NULL with a loss, logits
    clipped on both sides."""
    worst = 0.0
    for n_rows in ms.predict_sizes(k, _n_cu(rt)):
        for with_ids in (False, True):
            prob = ms.predict_problem(k, n_rows, with_ids)
            sel = prob["sel"]
            pairs = np.stack([prob["users"], prob["items"]], axis=1)[sel]
            want = ms.mf_predict_ld(pairs, *prob["params"], ms.B0)
            want_loss = float(ms.ips_logloss_ld(prob["y"][sel], want, prob["p"][sel]))
            what = f"k={k} rows={n_rows} ids={with_ids}"
            plain, _ = _twice(lambda: ms.run_predict(rt, prob, loss=False))
            fused, loss = _twice(lambda: ms.run_predict(rt, prob, loss=True))
            _, loss_only = _twice(lambda: ms.run_predict(rt, prob, loss=True, want_pred=False))
            worst = max(worst, ms.assert_scores_within(plain, want, ms.MF_TOL, what))
            np.testing.assert_array_equal(plain, fused)
            assert plain[0] == 1.0 and (n_rows == 1 or 0.0 < plain[1] < 1e-300), (what, plain[:2])  # clipped at +-700
            assert loss == pytest.approx(want_loss, rel=ms.LOSS_REL), what
            assert loss_only == loss, what
    print(f"distance predict k{k} {worst:.3e}")


# --------------------------------------------------------------------------
# e. through fit(): the schedule pipe and the smallest item caches end to end
# --------------------------------------------------------------------------
@pytest.mark.parametrize("k", ms.FIT_KS)
def test_fit_largest_factor_counts(k):
    import relevance_factorizationmachine_amd as pkg
    assert ms.capacity(k) == {513: 7, 1023: 3, 1024: 3}[k]
    rng = np.random.default_rng(k)
    nu, ni = 50, 8

    def log(m):
        pairs = np.stack([rng.integers(0, nu, size=m), (rng.zipf(1.3, size=m) - 1) % ni], axis=1).astype(np.int64)
        return {"features": pairs, "labels": (rng.random(m) < 0.5).astype(np.int64),
                "pscores": rng.uniform(0.1, 1.0, size=m) ** 0.5}
    train, val = log(1000), log(200)
    kw = dict(n_epochs=2, n_factors=k, lr=ms.LR, batch_size=300, seed=9, n_users=nu, n_items=ni, reg=ms.REG)
    model = pkg.LogisticMatrixFactorization(estimator="IPS", **kw)
    tr, va = model.fit(train, val)
    ref = cpu_ref.mf_fit(train, val, **kw)
    for nm in ("P", "Q", "b_u", "b_i"):
        assert rel_err(getattr(model, nm)(), ref[nm]) < TIGHT, nm
    assert rel_err(tr, ref["train_loss"]) < TIGHT and rel_err(va, ref["val_loss"]) < TIGHT
