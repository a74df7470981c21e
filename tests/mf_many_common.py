"""Shared by the tests of several MF models on one schedule (test_mf_many_host.py, test_gpu_mf_many.py):
what model m of a step test is, the batch of a case of mf_step_common.py as rows of a longer log in
shuffled order, a float64 statement of "M models on one schedule" with the three mistakes the
many-model kernels can make, a Python restatement of rfm_mf_many_geometry, and the raw ABI calls of
the many-model entry points with every array between sentinels.  Importing this module touches
neither the GPU nor the library under test.

Models.  Model m of a step test differs from its neighbours in everything it may differ in: init seed
``ms.INIT_SEED + m``, ``lr = ms.LR * (1 + m / 4)``, ``reg = ms.REG / (1 + m)``, ``b = ms.B0 + m / 10``,
and labels / propensities drawn as ``Case.ry`` draws them with the model index mixed into the seed.

Log.  The batch sits in a log of ``batch + 5`` rows in shuffled order, so ``ex_rows`` is not the
identity; a log row outside the batch holds ``OUTSIDE_RY``, which no update survives unnoticed.

Tolerance.  Nothing new: ``ms.MF_FLOOR`` / ``ms.MF_TOL`` as mf_step_common.py derives them."""
import contextlib
import zlib
from dataclasses import dataclass

import numpy as np

import mf_step_common as ms

EXTRA_ROWS = 5        # rows of the log outside the batch
OUTSIDE_RY = 1.0e6    # label / propensity of a log row that no record names


@dataclass
class Model:
    m: int
    lr: float
    reg: float
    b: float
    init: tuple          # (P, Q, b_u, b_i)
    ry_batch: np.ndarray  # label / propensity in batch order
    ry_log: np.ndarray    # ... as a vector over the log


def log_rows(case):
    """The log row of each batch position: the head of a permutation of ``batch + EXTRA_ROWS`` rows."""
    n = len(case.users)
    return np.random.default_rng(n + 17).permutation(n + EXTRA_ROWS)[:n].astype(np.int32)


def model_of(case, m, rows=None):
    from oracle import cpu_ref
    rows = log_rows(case) if rows is None else rows
    n = len(case.users)
    rng = np.random.default_rng([zlib.crc32(case.name.encode()), m])
    y, p = (rng.random(n) < 0.5).astype(np.float64), rng.uniform(0.1, 1.0, size=n) ** 0.5
    ry_log = np.full(n + EXTRA_ROWS, OUTSIDE_RY)
    ry_log[rows] = y / p
    return Model(m, ms.LR * (1 + m / 4), ms.REG / (1 + m), ms.B0 + m / 10,
                 cpu_ref.mf_init(ms.INIT_SEED + m, case.n_users, case.n_items, case.k), y / p, ry_log)


def models_of(case, n_models, rows=None):
    return [model_of(case, m, rows) for m in range(n_models)]


@contextlib.contextmanager
def constants_of(model):
    """``ms.run_levels_ex`` / ``ms.run_predict`` read B0, LR and REG of their module: this model's
    values for the duration."""
    saved = ms.B0, ms.LR, ms.REG
    ms.B0, ms.LR, ms.REG = model.b, model.lr, model.reg
    try:
        yield
    finally:
        ms.B0, ms.LR, ms.REG = saved


def oracle_of(case, model):
    """(P, Q, b_u, b_i) of one model after the batch, in long double."""
    return ms.mf_sgd_batch_ld(case.pairs, model.ry_batch, *model.init, model.b, model.lr, model.reg)


def reach_rows(case, rows=None):
    """The shared schedule of a case from rfm_mf_schedule_rows, with ``ms.reach``'s assertions that the
    case reaches the state it is named for: ``(ex, ex_rows, level_ptr, cache_items)``."""
    from relevance_factorizationmachine_amd.runtime import mf_schedule_rows
    rows = log_rows(case) if rows is None else rows
    ex0, lptr0, cache0 = ms.reach(case)
    cap = ms.capacity(case.k) if case.cache_cap is None else case.cache_cap
    ex, ex_rows, lptr, cache = mf_schedule_rows(case.users, case.items, rows, case.n_users, case.n_items, cap)
    for f in ("u", "i", "cslot", "gap"):
        np.testing.assert_array_equal(ex[f], ex0[f])
    np.testing.assert_array_equal(lptr, lptr0)
    np.testing.assert_array_equal(cache, cache0)
    assert np.isnan(ex["ry"]).all()
    return ex, ex_rows, lptr, cache


def records_of(ex, ex_rows, model):
    """The records of one model alone: what rfm_mf_schedule_ex gives for its labels and propensities."""
    own = ex.copy()
    own["ry"] = model.ry_log[ex_rows]
    return own


# --------------------------------------------------------------------------
# float64 statement of "M models on one schedule" and the mistakes a kernel can make of it
# --------------------------------------------------------------------------
MUTATIONS = ("neighbour_ry", "cache_to_model0", "rows_unpermuted")


def many_models_f64(case, sched, models, mutation=None):
    """Every model's (P, Q, b_u, b_i) after the shared schedule: ``ms.mf_sgd_batch_f64_reversed`` on the
    records in level order with that model's label / propensity, lr, reg, b and start.
    ``mutation``: "neighbour_ry" -- model 1 reads model 0's label / propensity vector;
    "cache_to_model0" -- model 1's cached item rows are written back into model 0's Q;
    "rows_unpermuted" -- record r reads log row r instead of ``ex_rows[r]``."""
    ex, ex_rows, lptr, cache = sched
    assert mutation in (None,) + MUTATIONS
    pairs = np.stack([ex["u"], ex["i"]], axis=1)
    out = []
    for mod in models:
        ry_log = models[0].ry_log if (mutation == "neighbour_ry" and mod.m == 1) else mod.ry_log
        rows = np.arange(len(ex)) if mutation == "rows_unpermuted" else ex_rows
        out.append(list(ms.mf_sgd_batch_f64_reversed(pairs, ry_log[rows], *mod.init, mod.b, mod.lr, mod.reg)))
    if mutation == "cache_to_model0":
        assert len(cache) and len(models) >= 2
        out[0][1][cache] = out[1][1][cache]
    return [tuple(o) for o in out]


def distance(got, want_ld):
    """Largest distance of (P, Q, b_u, b_i) from the oracle on the scale of ``ms.assert_params_within``."""
    rows = max(float(ms.row_distance(got[0], want_ld[0]).max()), float(ms.row_distance(got[1], want_ld[1]).max()))
    bias = max(float(ms.bias_distance(got[2], want_ld[2]).max()), float(ms.bias_distance(got[3], want_ld[3]).max()))
    return max(rows, bias)


# --------------------------------------------------------------------------
# rfm_mf_many_geometry restated from the constants of mf_step_common
# --------------------------------------------------------------------------
def geometry_py(n_models, k, n_recs, n_cu=ms.ASSUMED_CUS):
    lpr = ms.shape_class(k)[0]
    per_wg = ms.MF_BLOCK // lpr
    blocks = min(-(-n_recs // per_wg), ms.grid_pass(k, n_cu) // per_wg)
    return {"seq_threads": ms.seq_cap(k, "levels_ex") * lpr, "lanes_per_row": lpr, "seq_grid": n_models,
            "wide_grid_x": blocks, "wide_grid_y": n_models, "predict_grid_x": max(1, blocks),
            "predict_grid_y": n_models}


# --------------------------------------------------------------------------
# the raw ABI calls, every device array between sentinels
# --------------------------------------------------------------------------
class ModelTable:
    """The rfm_mf_model table of ``models`` on the device: each model's four arrays between sentinels
    (``ms.DeviceParams``), its label / propensity vector over the log (``ry_logs``; None: no vector)."""

    def __init__(self, rt, models, ry_logs=None):
        from relevance_factorizationmachine_amd import _lib
        self.rt, self.n = rt, len(models)
        self.params = [ms.DeviceParams(rt, *mod.init) for mod in models]
        self.ry = [ms.Guarded(rt, r, ms.PAD) for r in ry_logs] if ry_logs is not None else [None] * self.n
        rows = [_lib.MfModel(*p.ptrs(), r.ptr if r is not None else None, mod.b, mod.lr, mod.reg)
                for p, r, mod in zip(self.params, self.ry, models)]
        self.dev = rt.upload(np.frombuffer(bytes((_lib.MfModel * self.n)(*rows)), dtype=np.uint8).copy())

    @property
    def ptr(self):
        return self.dev.data_ptr()

    def host(self):
        """Every model's (P, Q, b_u, b_i); the sentinels around every array are checked."""
        self.rt.sync()
        for r in self.ry:
            if r is not None:
                r.host()
        return [p.host() for p in self.params]


def run_levels_many(rt, case, sched, models):
    """rfm_mf_sgd_levels_many on the shared schedule of ``reach_rows``: every model's (P, Q, b_u, b_i)."""
    from relevance_factorizationmachine_amd import _lib
    ex, ex_rows, lptr, cache = sched
    table = ModelTable(rt, models, [mod.ry_log for mod in models])
    d_ex = rt.upload(np.ascontiguousarray(ex).view(np.uint8))
    d_rows, d_lptr = rt.upload(ex_rows), rt.upload(lptr)
    d_cache = rt.upload(cache) if len(cache) else None
    _lib.check(rt.lib.rfm_mf_sgd_levels_many(
        rt.ctx, d_ex.data_ptr(), d_rows.data_ptr(), lptr.ctypes.data, d_lptr.data_ptr(), len(lptr) - 1,
        d_cache.data_ptr() if len(cache) else None, len(cache), table.ptr, len(models), case.k))
    return table.host()


def run_levels_alone(rt, case, sched, model):
    """rfm_mf_sgd_levels_ex on one model's own records (``ms.run_levels_ex`` with that model's values)."""
    ex, ex_rows, lptr, cache = sched
    with constants_of(model):
        return ms.run_levels_ex(rt, case, (records_of(ex, ex_rows, model), lptr, cache), model.init)


LOSS_STRIDE = 3  # a neighbour's loss slot is a sentinel
OUT_OFFSET = 5   # elements the calls of run_predict_many add to every model's base pointer


def run_predict_many(rt, prob, models, labels, loss):
    """rfm_mf_predict_many (``loss`` False) or rfm_mf_predict_loss_many with scores on ``models`` and
    their ``labels`` [(y, p) over the log]: ``([scores of model m], [loss of model m] or None)``.  Each
    score buffer has 8 more elements than rows and starts ``OUT_OFFSET`` elements into its allocation."""
    from relevance_factorizationmachine_amd import _lib
    n, M = prob["n_rows"], len(models)
    table = ModelTable(rt, models)
    du, di = rt.upload(prob["users"].astype(np.int32)), rt.upload(prob["items"].astype(np.int32))
    d_ids = rt.upload(prob["ids"]) if prob["ids"] is not None else None
    ids_ptr = d_ids.data_ptr() if d_ids is not None else None
    outs = [ms.Guarded.blank(rt, n + 8, pad=ms.PAD + OUT_OFFSET) for _ in range(M)]
    # the table names the allocation's interior OUT_OFFSET elements early; the call adds them back
    d_base = rt.upload(np.asarray([o.ptr - 8 * OUT_OFFSET for o in outs], dtype=np.uint64))
    if not loss:
        _lib.check(rt.lib.rfm_mf_predict_many(rt.ctx, du.data_ptr(), di.data_ptr(), ids_ptr, n, table.ptr, M,
                                              prob["k"], d_base.data_ptr(), OUT_OFFSET))
        losses = None
    else:
        keep = [(rt.upload(y), rt.upload(p)) for y, p in labels]
        rows = [_lib.MfLabels(y.data_ptr(), p.data_ptr()) for y, p in keep]
        d_labels = rt.upload(np.frombuffer(bytes((_lib.MfLabels * M)(*rows)), dtype=np.uint8).copy())
        d_loss = ms.Guarded.blank(rt, (M - 1) * LOSS_STRIDE + 1)
        _lib.check(rt.lib.rfm_mf_predict_loss_many(
            rt.ctx, du.data_ptr(), di.data_ptr(), d_labels.data_ptr(), ids_ptr, n, table.ptr, M, prob["k"],
            ms.LOSS_EPS, d_base.data_ptr(), OUT_OFFSET, d_loss.ptr, LOSS_STRIDE))
    after = table.host()  # (synchronises; the parameters are inputs here and must not change)
    for got, mod in zip(after, models):
        for a, b in zip(got, mod.init):
            np.testing.assert_array_equal(a, b)
    scores = [o.host(written=n)[:n] for o in outs]
    if loss:
        flat = d_loss.host()
        bits = flat.view(np.uint64)
        between = np.ones(len(flat), dtype=bool)
        between[::LOSS_STRIDE] = False
        assert (bits[between] == ms.SENTINEL_BITS).all(), "a loss was written between the models' slots"
        losses = [float(v) for v in flat[::LOSS_STRIDE]]
    return scores, losses


def predict_models(prob, n_models):
    """Models and labels of a scoring problem of ``ms.predict_problem``: model 0 is the problem's own;
    the others have parameters of another init seed (the two clipped rows kept) and labels /
    propensities of their own."""
    from oracle import cpu_ref
    nu, ni = prob["params"][0].shape[0], prob["params"][1].shape[0]
    models, labels = [], []
    for m in range(n_models):
        if m == 0:
            params, y, p = prob["params"], prob["y"], prob["p"]
        else:
            P, Q, bu, bi = cpu_ref.mf_init(ms.INIT_SEED + m, nu, ni, prob["k"])
            bu[0], bu[1] = 900.0, -900.0
            rng = np.random.default_rng([prob["k"], prob["n_rows"], m])
            y = (rng.random(len(prob["y"])) < 0.5).astype(np.float64)
            p = rng.uniform(0.1, 1.0, size=len(y)) ** 0.5
            params = (P, Q, bu, bi)
        models.append(Model(m, ms.LR, ms.REG, ms.B0 + m / 10, params, None, None))
        labels.append((y, p))
    return models, labels


def predict_alone(rt, prob, model, label, loss):
    """``ms.run_predict`` on one model alone."""
    own = dict(prob, params=model.init, y=label[0], p=label[1])
    with constants_of(model):
        return ms.run_predict(rt, own, loss)


class ValEvaluatorLike:
    """The attributes of the reference's ValEvaluator (utils/evaluate.py:22-33,160-207) with the
    oracle's restatement as its evaluate(), as tests/test_gpu_eval.py builds it."""

    metric_name = "DCG"
    rfm_device_evaluator = True  # opts in: its evaluate() IS the reference's metric

    def __init__(self, frame, features, k=5):
        self.k, self.features, self.interaction_df, self.calls = k, features, frame, 0

    def evaluate(self, y_scores, estimator):
        from oracle import cpu_ref
        self.calls += 1
        return cpu_ref.val_dcg(self.interaction_df, y_scores, estimator, k=self.k)
