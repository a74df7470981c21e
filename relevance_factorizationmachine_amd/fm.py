"""``FactorizationMachines`` with the reference's surface (``src/fm.py:17-133``)
on top of the HIP kernels of librfm_hip.so.

Same dataclass fields, same ``fit(train, val) -> (train_loss, val_loss)`` and
``predict(X)`` / ``predict(X=...)``, same side attributes (``val_metrics``,
``model_name`` when an evaluator is given; ``w0``, ``w``, ``V`` callables).  The
host only prepares inputs (parameter init with the reference's NumPy calls,
mini-batch ids, uploads) and enqueues; every floating-point operation of the
loop runs in the kernels of ``csrc/rfm_fm.hip``.

Beyond the reference: the catalogue methods (``recommend.py``) and fold-in of
users and items that arrive after the fit (``fold_in_users`` / ``fold_in_items``
/ ``append_columns``, ``csrc/rfm_fm_fold.hip``, the host side shared with MF in
``fold.py``).
"""
from __future__ import annotations

import ctypes as C
import weakref
from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib, fold
from .base import LOSS_EPS, PointwiseBaseRecommender
from .evaluate import EvalLoop, FitHook, device_frame, runs
from .optimizer import DeviceSGD, take_optimizer
from .runtime import BatchIdStream, CsrCache, DeviceCSR, Runtime


class _PlanCache:
    """The last few training plans of a device, by the identity of the device copies they were
    built from (log, labels, propensities) and their shape parameters: a second model fitted on
    the same split with the same factor count and batch size takes the plan as it is (a plan
    holds no model state).  A plan that is lent out is not lent twice."""

    CAPACITY = 2

    def __init__(self):
        self._items = []  # [key, (weakrefs), plan, busy]

    def take(self, rt, csr, y, p, n_factors: int, max_batch: int, hot_min_count: int) -> "FmPlan":
        key = (id(csr), id(y), id(p), n_factors, max_batch, hot_min_count)
        for item in self._items:
            if item[0] == key and not item[3] and all(r() is o for r, o in zip(item[1], (csr, y, p))):
                item[3] = True
                return item[2]
        plan = FmPlan(rt, csr, y, p, n_factors, max_batch, hot_min_count)
        try:
            refs = tuple(weakref.ref(o) for o in (csr, y, p))
        except TypeError:
            return plan  # not remembered: give_back() closes it
        self._items.append([key, refs, plan, True])
        while len(self._items) > self.CAPACITY:
            for i, item in enumerate(self._items):
                if not item[3]:
                    self._items.pop(i)[2].close()
                    break
            else:
                break
        return plan

    def give_back(self, plan: "FmPlan") -> None:
        for item in self._items:
            if item[2] is plan:
                item[3] = False
                return
        plan.close()

    def clear(self) -> None:
        for item in [i for i in self._items if not i[3]]:
            self._items.remove(item)
            item[2].close()


def plan_cache(rt: Runtime) -> _PlanCache:
    if getattr(rt, "_plan_cache", None) is None:
        rt._plan_cache = _PlanCache()
    return rt._plan_cache


class FmPlan:
    """Owner of an ``rfm_fm_plan`` (column-major view of a training CSR)."""

    def __init__(self, rt: Runtime, csr: DeviceCSR, labels, pscores, n_factors: int, max_batch: int,
                 hot_min_count: int = 0):
        """``labels`` / ``pscores``: host arrays, or float64 device tensors the caller already
        holds.  The plan is built on the device from the device copy of the log."""
        self.rt = rt
        y = labels if hasattr(labels, "data_ptr") else rt.upload(np.asarray(labels), dtype=np.float64)
        p = pscores if hasattr(pscores, "data_ptr") else rt.upload(np.asarray(pscores), dtype=np.float64)
        if y.shape[0] != csr.shape[0] or p.shape[0] != csr.shape[0]:
            raise ValueError("labels / pscores do not match the number of rows")
        handle = C.c_void_p()
        _lib.check(rt.lib.rfm_fm_plan_create_device(
            rt.ctx, csr.indptr.data_ptr(), csr.indices.data_ptr(), csr.values.data_ptr(),
            y.data_ptr(), p.data_ptr(), csr.shape[0], csr.shape[1], n_factors, max_batch,
            hot_min_count, C.byref(handle)))
        self.handle = handle

    def info(self) -> dict:
        out = np.zeros(8, dtype=np.int64)
        _lib.check(self.rt.lib.rfm_fm_plan_info(self.handle, out.ctypes.data))
        return dict(zip(("tasks", "split_columns", "hot_columns", "nnz", "device_bytes",
                         "forward_workgroups", "slots", "task_words"), (int(v) for v in out)))

    def layout(self) -> dict:
        out = np.zeros(4, dtype=np.int32)
        _lib.check(self.rt.lib.rfm_fm_plan_layout(self.handle, out.ctypes.data))
        return dict(zip(("row_blocks", "row_block_bytes", "lanes_per_row", "longest_row"),
                        (int(v) for v in out)))

    def sliced(self) -> dict:
        """The sliced loss forwards of ``rfm_fm_train`` (even factor counts above 128)."""
        out = np.zeros(4, dtype=np.int32)
        _lib.check(self.rt.lib.rfm_fm_plan_sliced(self.handle, out.ctypes.data))
        return dict(zip(("slices", "factors_per_slice", "cached_columns", "records_per_row"),
                        (int(v) for v in out)))

    def hot_columns(self) -> np.ndarray:
        out = np.zeros(max(self.info()["hot_columns"], 1), dtype=np.int32)
        _lib.check(self.rt.lib.rfm_fm_plan_hot_columns(self.handle, out.ctypes.data, out.shape[0]))
        return out[: self.info()["hot_columns"]]

    def sliced_columns(self) -> np.ndarray:
        """The columns a sliced forward's workgroup keeps in LDS, in their LDS order."""
        n = self.sliced()["cached_columns"]
        out = np.zeros(max(n, 1), dtype=np.int32)
        _lib.check(self.rt.lib.rfm_fm_plan_sliced_columns(self.handle, out.ctypes.data, out.shape[0]))
        return out[:n]

    def sliced_geometry(self, n_rows: int, form_rows: int = -1) -> dict:
        """The launch a sliced forward of ``n_rows`` rows takes (``rfm_fm_sliced_geometry``)."""
        out = np.zeros(4, dtype=np.int32)
        _lib.check(self.rt.lib.rfm_fm_sliced_geometry(self.rt.ctx, self.handle, int(n_rows), int(form_rows),
                                                      out.ctypes.data))
        return dict(zip(("sliced", "workgroups", "rows_per_workgroup", "lds_bytes"), (int(v) for v in out)))

    def step_form(self, batch: int, n_riding_rows: int = 0) -> dict:
        """The forward launch of a step of ``batch`` rows on this plan (``rfm_fm_step_form``); ``kind`` is
        one of ``_lib.FWD_KINDS``."""
        out = np.zeros(8, dtype=np.int32)
        _lib.check(self.rt.lib.rfm_fm_step_form(self.rt.ctx, self.handle, int(batch), int(n_riding_rows),
                                                out.ctypes.data))
        form = dict(zip(("block", "workgroups", "trip", "lanes", "kind", "lanes8", "lds_bytes", "fixed_order"),
                        (int(v) for v in out)))
        form["kind"] = _lib.FWD_KINDS[form["kind"]]
        return form

    def set_optimizer(self, kind: int, acc_w0=None, acc_w=None, acc_V=None, eps: float = 0.0) -> None:
        """The update rule of the plan's steps (``rfm_fm_plan_set_optimizer``): ``_lib.OPT_SGD``, or
        ``_lib.OPT_ADAGRAD`` with the three accumulators (device tensors the caller keeps alive)."""
        ptr = [t.data_ptr() if t is not None else None for t in (acc_w0, acc_w, acc_V)]
        _lib.check(self.rt.lib.rfm_fm_plan_set_optimizer(self.handle, int(kind), *ptr, float(eps)))

    def optimizer(self) -> int:
        out = np.zeros(1, dtype=np.int32)
        _lib.check(self.rt.lib.rfm_fm_plan_optimizer(self.handle, out.ctypes.data))
        return int(out[0])

    def close(self) -> None:
        if self.handle is not None:
            self.rt.lib.rfm_fm_plan_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class FmFit:
    """What a fit of FM holds on the device -- the split, the training plan, the two loss lists --
    and the arguments that every training entry of the library shares (``rfm_fm_train``,
    ``rfm_fm_train_part``, ``rfm_fm_train_eval``, ``rfm_fm_fit_dp``, ``rfm_fm_fit_dp_eval``).

    ``cached``: the uploads and the plan come from the runtime's caches (``log_cache``,
    ``upload_cached``, ``plan_cache``; subject to ``Runtime.remember_splits``) -- the single-GPU
    fit, whose drivers fit several models on one split; else plain uploads and a plan of its own
    (``dist.HipDpEngine``: ``max_batch`` is the largest shard)."""

    def __init__(self, model, train: dict, val: dict, max_batch: int, cached: bool):
        rt = self.rt = model._rt
        self.model = model
        self.keep = keep = cached and rt.remember_splits

        # a log that is already in HBM (features.assemble / load_csr_to_device) is used as it is
        # (cached: device copies of the split are remembered per device; an array edited in place
        # is uploaded again -- CsrCache._fingerprint)
        def log(X):
            return X if isinstance(X, DeviceCSR) else (rt.log_cache().get(X) if keep else DeviceCSR(rt, X))

        def vec(a):
            return rt.upload_cached(a, np.float64) if keep else rt.upload(np.asarray(a), dtype=np.float64)

        self.tr, self.y, self.p = log(train["features"]), vec(train["labels"]), vec(train["pscores"])
        self.va, self.vy, self.vp = log(val["features"]), vec(val["labels"]), vec(val["pscores"])
        hot = -2 if model.deterministic else model.hot_min_count
        plan_args = (rt, self.tr, self.y, self.p, model.n_factors, max_batch, hot)
        self.plan = plan_cache(rt).take(*plan_args) if keep else FmPlan(*plan_args)
        self.tl = rt.empty((model.n_epochs,), self.y.dtype)
        self.vl = rt.empty((model.n_epochs,), self.y.dtype)
        # an empty validation set: the reference's mean over no rows is nan (src/base.py:61)
        self.has_val = self.va.shape[0] > 0
        if not self.has_val:
            self.vl.fill_(float("nan"))

    def ids_ptr(self, first: int, chunk_first: int, dev_ids) -> int:
        """Address of iteration ``first``'s batch in ``dev_ids``, the ids from ``chunk_first`` on."""
        return dev_ids.data_ptr() + (first - chunk_first) * self.model.batch_size * 4

    def tail(self, first: int) -> tuple:
        """The arguments every training entry ends its own with, for a run that starts at ``first``:
        parameters, step size, validation split, and where the two losses go."""
        m, va = self.model, self.va
        return (m.w0.dev.data_ptr(), m.w.dev.data_ptr(), m.V.dev.data_ptr(), float(m.lr),
                va.indptr.data_ptr(), va.indices.data_ptr(), va.values.data_ptr(),
                self.vy.data_ptr(), self.vp.data_ptr(), va.shape[0], LOSS_EPS,
                self.tl.data_ptr() + first * 8, self.vl.data_ptr() + first * 8 if self.has_val else None)

    def losses(self) -> tuple:
        return self.tl.cpu().numpy().tolist(), self.vl.cpu().numpy().tolist()

    def release(self) -> None:
        if self.keep:
            plan_cache(self.rt).give_back(self.plan)
        else:
            self.plan.close()


@dataclass
class FoldedColumns:
    """The id columns of new rows of one side of a trained FM model (``fold_in_users`` /
    ``fold_in_items``): device tensors ``w [n_new]`` and ``V [n_new, k]`` (the new
    columns' weights and factor rows) and the served operands of the grown rows, ``A [n_new, kpad]``
    and ``L [n_new]`` (``recommend.Operands``); ``side`` "user" or "item".  ``features``: the rows' own
    feature entries, the canonical host CSR ``[n_new, n_features]`` they were folded with
    (``recommend.grown_side_sums`` serves folded items from it)."""

    side: str
    w: object
    V: object
    A: object
    L: object
    rt: Runtime
    features: object = None

    def __len__(self) -> int:
        return int(self.w.shape[0])

    def numpy(self):
        """``(V, w)`` on the host, after the work enqueued so far."""
        self.rt.sync()
        return self.V.cpu().numpy(), self.w.cpu().numpy()


def fold_rows(sides, new_rows, side: int, n_features: int):
    """The feature entries of the new rows of ``side`` (0: users, 1: items) as a canonical CSR
    ``[n_new, n_features]`` (host only).  ``ValueError`` for another width, and for a column that
    the OTHER side of ``sides`` stores: the pair rows would not be user row + item row."""
    from . import recommend as rec

    if len(new_rows.shape) != 2 or int(new_rows.shape[1]) != int(n_features):
        raise ValueError(f"new_rows of shape {tuple(new_rows.shape)} for a model of {int(n_features)} columns")
    X = new_rows.tocsr()
    if not X.has_canonical_format:
        X = X.copy()
        X.sum_duplicates()
    both = np.intersect1d(rec._stored_columns(X), rec._stored_columns(sides._host[1 - side]))
    if both.size:
        raise ValueError(f"column {int(both[0])} of new_rows is stored on the {('item', 'user')[side]} side "
                         f"({both.size} such columns): pair rows are not user_rows[u] + item_rows[i]")
    return X


@dataclass
class FactorizationMachines(PointwiseBaseRecommender):
    """Factorization Machines trained by mini-batch SGD on an MI355X.

    Args (``src/fm.py:20-29``):
    - n_features (int): number of feature columns
    - alpha (float): scale of the uniform initialisation
    - evaluator: optional object with ``.features["FM"]`` and
      ``.evaluate(y_scores=, estimator=)`` (the reference's ``ValEvaluator``)
    """

    n_features: int
    alpha: float = 2.0
    evaluator: Optional[object] = None

    # Not a constructor argument: columns with at least this many expected
    # entries per batch are summed on chip (0 = library default; -1 = never, which makes
    # every sum's order fixed and a fit bitwise reproducible; -2 = the default columns, summed
    # on chip in a fixed order: rfm_hip.h).
    hot_min_count = 0
    # Not a constructor argument: True = every sum in a fixed order, i.e. hot_min_count = -2
    # (a fit is then bitwise reproducible, at 1.1-1.25x the step time on KuaiRec-shaped logs).
    deterministic = False
    # Not a constructor argument: a ValEvaluator-like ``evaluator`` (see evaluate.py) is
    # computed on the device; False keeps the host callback for every evaluator.
    device_evaluator = True
    # Not a constructor argument: True samples the mini-batch ids on the device
    # (runtime.sample_batches_device, bit-identical to the host sampler) instead of on the host
    # cores; fit() and dist.fit_data_parallel honour it.  Off by default until it outruns the
    # host threads on a cold fit.
    device_sampler = False
    # Not constructor arguments: the update rule of fit() -- "sgd" (the reference's, theta -= lr * g)
    # or "adagrad" (G += g * g; theta -= lr * g / (sqrt(G) + adagrad_eps), accumulators G of the
    # parameters' shapes that start at adagrad_init and persist across fit() calls: DESIGN §8 N19).
    # The data-parallel fit and fold-in take the SGD step only.
    optimizer = "sgd"
    adagrad_eps = 1e-10
    adagrad_init = 0.0

    def __post_init__(self) -> None:
        # src/fm.py:31-53 -- the reference's NumPy calls, in its draw order
        np.random.seed(self.seed)
        w0 = np.array([0.0])
        limit = self.alpha * np.sqrt(6 / self.n_features)
        w = np.random.uniform(low=-limit, high=limit, size=self.n_features)
        limit = self.alpha * np.sqrt(6 / self.n_factors)
        V = np.random.uniform(low=-limit, high=limit, size=(self.n_features, self.n_factors))

        self._rt = Runtime.get()
        self.w0 = DeviceSGD(self._rt, w0, self.lr)
        self.w = DeviceSGD(self._rt, w, self.lr)
        self.V = DeviceSGD(self._rt, V, self.lr)
        self._csr_cache = CsrCache(self._rt)

        if self.evaluator is not None:
            self.val_metrics = []
            self.model_name = "FM"

    # ------------------------------------------------------------------ fit
    def fit(self, train: dict, val: dict) -> tuple:
        """src/fm.py:55-112.  One "epoch" is one mini-batch step; returns the
        per-iteration train and validation IPS log-loss as two lists."""
        rt = self._rt
        X = train["features"]
        n_rows = X.shape[0]
        if X.shape[1] != self.n_features:
            raise ValueError(f"train features have {X.shape[1]} columns, model has {self.n_features}")
        take_optimizer(self, ("w0", "w", "V"))
        if self.n_epochs <= 0:
            return [], []
        # batch selection: resample(..., random_state=epoch) (src/fm.py:72-79), sampled chunk by
        # chunk on the host (or on the sampler stream: device_sampler) while the GPU trains on
        # the chunk before
        id_stream = BatchIdStream(rt, n_rows, self.batch_size, self.n_epochs, need_host=False,
                                  device_sampler=self.device_sampler)
        try:
            return self._fit(train, val, id_stream)
        finally:
            id_stream.close()  # (its sampler thread runs from the constructor on)

    def _fit(self, train: dict, val: dict, id_stream: BatchIdStream) -> tuple:
        rt = self._rt
        st = FmFit(self, train, val, self.batch_size, cached=True)
        plan, tr, va = st.plan, st.tr, st.va
        self.plan_info = dict(plan.info(), **plan.layout(), **plan.sliced())  # (what the last fit trained with)
        if st.has_val:  # (the split's device copy does not change during this fit)
            _lib.check(rt.lib.rfm_fm_plan_register_log(
                rt.ctx, plan.handle, 0, va.indptr.data_ptr(), va.indices.data_ptr(), va.values.data_ptr(),
                va.shape[0]))

        def make_loop(evaluator):
            # ValEvaluator's IPS-DCG@k from the scores in HBM (rfm_val_dcg), inside the library's
            # loop (rfm_fm_train_eval); only the users whose value hangs on the order of tied
            # scores are redone on the host
            ev_X = evaluator.features[self.model_name]
            frame = device_frame(rt, evaluator, self.estimator, ev_X.shape[0])
            if frame is None:
                return None
            if ev_X.shape[1] != self.n_features:
                raise ValueError(f"X has {ev_X.shape[1]} columns, model has {self.n_features}")
            ev = self._csr_cache.get(ev_X)
            _lib.check(rt.lib.rfm_fm_plan_register_log(
                rt.ctx, plan.handle, 1, ev.indptr.data_ptr(), ev.indices.data_ptr(), ev.values.data_ptr(),
                ev.shape[0]))
            return EvalLoop(rt, frame, evaluator, self.estimator, self.n_epochs, log=ev)

        try:
            if take_optimizer(self, ("w0", "w", "V")):
                # (plans are shared through plan_cache: the rule is set for this fit and taken back below)
                plan.set_optimizer(_lib.OPT_ADAGRAD, self.w0.acc, self.w.acc, self.V.acc, self.adagrad_eps)
            hook = FitHook(self, self.n_epochs, self.predict, make_loop)
            for first, host_ids, dev_ids in id_stream.chunks():
                count = dev_ids.shape[0]
                # one enqueue per run of iterations: the whole chunk without an evaluator, else up
                # to the next evaluation point, the end of the chunk of score slots, or one
                # iteration for a host callback (FitHook.limit)
                for at, n in runs(first, count, hook.limit):
                    args = (rt.ctx, plan.handle, tr.indptr.data_ptr(), tr.indices.data_ptr(), tr.values.data_ptr(),
                            st.y.data_ptr(), st.p.data_ptr(), st.ids_ptr(at, first, dev_ids), self.batch_size, n,
                            *st.tail(at))
                    if hook.cat is not None:
                        # a piece of the call of `count` iterations that a fit without an evaluator
                        # makes: the same loss forms, hence the same losses bit for bit
                        _lib.check(rt.lib.rfm_fm_train_part(*args, count))
                    elif hook.loop is not None:
                        _lib.check(rt.lib.rfm_fm_train_eval(*args, *hook.loop.call_args(at)))
                    else:
                        _lib.check(rt.lib.rfm_fm_train(*args))
                    hook.ran(at, n)
            rt.sync()
            hook.finish()
        finally:
            rt.sync()
            # (the registration ends with the fit: the plan may outlive this split's device copy)
            for log_slot in (0, 1):
                rt.lib.rfm_fm_plan_register_log(rt.ctx, plan.handle, log_slot, None, None, None, 0)
            rt.lib.rfm_fm_plan_set_optimizer(plan.handle, _lib.OPT_SGD, None, None, None, 0.0)
            st.release()
        return st.losses()

    # -------------------------------------------------------------- predict
    def predict(self, X) -> np.ndarray:
        """src/fm.py:114-133 -- scores of the rows of a sparse matrix."""
        rt = self._rt
        if X.shape[1] != self.n_features:
            raise ValueError(f"X has {X.shape[1]} columns, model has {self.n_features}")
        dev = X if isinstance(X, DeviceCSR) else self._csr_cache.get(X)
        n = dev.shape[0]
        out = rt.empty((n,), self.w.dev.dtype)
        _lib.check(rt.lib.rfm_fm_forward(
            rt.ctx, dev.indptr.data_ptr(), dev.indices.data_ptr(), dev.values.data_ptr(), None, n,
            self.w0.dev.data_ptr(), self.w.dev.data_ptr(), self.V.dev.data_ptr(),
            self.n_features, self.n_factors, out.data_ptr()))
        rt.sync()
        return out.cpu().numpy()

    # -------------------------------------------------------------- fold-in
    def _fold_in(self, side: int, sides, new_rows, data: dict, n_passes: int, init, lr, ops, group=None,
                 check=True) -> FoldedColumns:
        """The id columns of new rows of ``side`` (0: users, 1: items) trained against the fixed
        other side (``rfm_fm_fold_in``): every check on the host first, then the
        side sums of ``new_rows`` and the fold launch enqueued on the runtime's stream, no host wait."""
        from . import recommend as rec

        n_users, n_items = rec.catalogue_shape(self, sides)
        kf, kp = int(self.n_factors), rec.pad4(self.n_factors)
        X = fold_rows(sides, new_rows, side, self.n_features)
        n_new, n_fixed = int(X.shape[0]), (n_items, n_users)[side]
        examples = fold.grouped_examples(self._rt, data, n_new, n_fixed, side, n_passes, group, check)
        lr = float(self.lr if lr is None else lr)
        start = fold.initial_state(init, n_new, kf, ("V", "w"))
        if ops is not None and (tuple(ops.A.shape) != (n_users, kp) or tuple(ops.B.shape) != (n_items, kp)):
            raise ValueError(f"ops of {tuple(ops.A.shape)}, {tuple(ops.B.shape)} for sides of {n_users} users and "
                             f"{n_items} items at {kf} factors")
        import torch

        rt = self._rt
        if start is None:
            V_new = torch.zeros((n_new, kf), dtype=torch.float64, device=rt.torch_device)
            w_new = torch.zeros((n_new,), dtype=torch.float64, device=rt.torch_device)
        else:
            V_new, w_new = rt.upload(start[0]), rt.upload(start[1])
        A_new, L_new = rt.empty((n_new, kp), torch.float64), rt.empty((n_new,), torch.float64)
        if n_new:
            if ops is None:
                ops = rec.operands(self, sides)
            F, fL = ((ops.B, ops.LI), (ops.A, ops.LU))[side]
            g, l = rec.side_sums(rt, DeviceCSR(rt, X), self.w.dev, self.V.dev, self.n_features, kf)
            dev = examples()
            _lib.check(rt.lib.rfm_fm_fold_in(
                rt.ctx, *(d.data_ptr() for d in dev), n_new, g.data_ptr(), l.data_ptr(), F.data_ptr(), fL.data_ptr(),
                n_fixed, self.w0.dev.data_ptr(), kf, lr, int(n_passes), w_new.data_ptr(), V_new.data_ptr(),
                A_new.data_ptr(), L_new.data_ptr()))
        return FoldedColumns(("user", "item")[side], w_new, V_new, A_new, L_new, rt, X)

    def fold_in_users(self, sides, new_rows, data: dict, n_passes: int, init=None, lr=None, ops=None, group=None,
                      check=True) -> FoldedColumns:
        """Id columns for users who arrived after the fit: each new user's one-hot
        id column -- its weight and factor row -- is learned from the user's interactions by the
        reference's batch-sum step (``src/fm.py:80-88``) with the trained model held fixed.  That is
        the SGD step whatever ``optimizer`` the model was fitted with: a new column has no history
        of gradients, and ``append_columns`` starts its accumulators at ``adagrad_init``.
        ``sides``: the catalogue the model serves; ``new_rows``: CSR ``[n_new, n_features]`` of the
        new users' FEATURE entries (a column stored on the item side is a ``ValueError``); ``data``
        as ``fit()`` of the MF model takes it: ``features`` ``(N, 2)`` of ``[user, item]`` with
        new-user indices 0..n_new-1 in the user column and item rows of ``sides`` in the item
        column, ``labels``, ``pscores``.  One pass is one full-batch step over a user's examples;
        ``lr``: the model's unless given; ``init``: ``(V [n_new, k], w [n_new])`` to start from
        (default zeros); ``ops``: ``recommend.operands(self, sides)`` to reuse.  The model is not
        written; serve the result through ``new_users=`` or ``append_columns`` it.  ``group``, ``check``:
        where the examples are grouped by user and whether the device's id check is waited for, as
        ``LogisticMatrixFactorization.fold_in_users`` takes them."""
        return self._fold_in(0, sides, new_rows, data, n_passes, init, lr, ops, group, check)

    def fold_in_items(self, sides, new_rows, data: dict, n_passes: int, init=None, lr=None, ops=None, group=None,
                      check=True) -> FoldedColumns:
        """``fold_in_users`` with the sides exchanged: ``new_rows`` holds new items' feature entries,
        the item column of ``features`` new-item indices and the user column user rows of ``sides``."""
        return self._fold_in(1, sides, new_rows, data, n_passes, init, lr, ops, group, check)

    def append_columns(self, folded: FoldedColumns) -> np.ndarray:
        """Grows ``w``, ``V`` and ``n_features`` by folded id columns, at the end (and, under
        ``optimizer = "adagrad"``, their accumulators by rows of ``adagrad_init``); returns their
        column ids.  Rows that store those columns (entry 1 next to the row's feature entries) are
        then scored by ``predict``, served by the catalogue methods on a ``Sides`` of the grown
        width and trained by a further ``fit``; where a loader's id segment sits is the loader's
        business, nothing is inserted mid-matrix."""
        if not isinstance(folded, FoldedColumns):
            raise TypeError("append_columns takes the FoldedColumns of fold_in_users / fold_in_items")
        if tuple(folded.V.shape[1:]) != (int(self.n_factors),):
            raise ValueError(f"folded columns of {tuple(folded.V.shape)} for a model of {int(self.n_factors)} factors")
        first = int(self.n_features)
        self.w.append(folded.w)
        self.V.append(folded.V)
        self.n_features = first + len(folded)
        # (matrices of the old width are refused from here on; training plans are keyed on the log
        # they were built from, and a log of the grown width is another log)
        self._csr_cache = CsrCache(self._rt)
        return np.arange(first, first + len(folded))

    # ------------------------------------------------------------ catalogue
    # new_users: the FoldedColumns of fold_in_users stand in for the user side -- ``users`` and
    # ``exclude`` then index the folded rows, and the model is not touched
    def score_pairs(self, sides, users=None, new_users=None) -> np.ndarray:
        """``predict()`` of every (user, item) pair of ``sides`` (``recommend.Sides``) as a
        ``[n_users (or len(users)), n_items]`` matrix, without the pairs' design matrix: side
        sums + one dense product (recommend.py; src/fm.py:114-133 restated)."""
        from . import recommend as rec

        return rec.score_pairs(*rec.operands(self, sides, new_users=new_users), users)

    def recommend(self, sides, k: int, users=None, exclude=None, new_users=None):
        """The ``k`` (1..64) best items of the catalogue per user: ``(items int32 [n, k], scores
        float64 [n, k])``, ranked by logit (ties: higher item index first), scores as
        ``predict()`` gives them; ``exclude``: items never to return, CSR by user id."""
        from . import recommend as rec

        return rec.topk(*rec.operands(self, sides, new_users=new_users), k, users, exclude)

    def rank_items(self, sides, users, items, exclude=None, new_users=None):
        """Where the pairs ``(users[n], items[n])`` land in their users' ranking of the whole
        catalogue of ``sides``: ``(ranks int32 [n], scores float64 [n], candidates int32 [n])`` in
        input order -- ``ranks`` 0-based under ``recommend()``'s order among the user's
        ``candidates`` (logit not NaN, not in ``exclude``), at any depth (recommend.py)."""
        from . import recommend as rec

        return rec.rank_items(*rec.operands(self, sides, new_users=new_users), users, items, exclude)

    def rank_catalogue(self, sides, depth: int, users=None, exclude=None, new_users=None):
        """Every user's ranking of the catalogue of ``sides`` down to ``depth`` (any integer >= 1;
        ``depth >= n_items``: the full ordering): ``(items int32 [n, depth], scores float64
        [n, depth], n_ranked int32 [n])`` under ``recommend()``'s order, short rows padded with
        item -1 / score NaN; the first 64 columns are ``recommend(k=64)``'s (recommend.py)."""
        from . import recommend as rec

        return rec.rank_catalogue(*rec.operands(self, sides, new_users=new_users), depth, users, exclude)

    def recommend_diverse(self, sides, k: int, depth=None, trade_off=0.5, users=None, exclude=None, metric="cosine",
                          item_penalty=None, new_users=None):
        """``k`` (1..64) of each user's ``depth`` best items of ``sides`` (default ``min(n_items, max(64,
        4 k))``, at most 1 024), chosen greedily by Maximal Marginal Relevance: ``(items int32 [n, k],
        scores float64 [n, k], values float64 [n, k])`` in the order chosen.  A pick maximises
        ``trade_off * score - item_penalty[item] - (1 - trade_off) * max similarity to the picks before
        it``, the similarity the cosine (``metric="dot"``: the dot product) of the item vectors ``b_i``;
        ``trade_off=1`` without a penalty is ``recommend(k)``.  An item without entries has no
        direction: its similarity to anything counts as 0.  Short rows pad with item -1 / NaN
        (recommend.diverse)."""
        from . import recommend as rec

        return rec.diverse(self, sides, k, depth, trade_off, users, exclude, metric, item_penalty, new_users)

    # the item -> users direction.  new_items: the FoldedColumns of fold_in_items
    # stand in for the item side -- ``items`` and the item axis of ``exclude`` then index the folded
    # rows; new_users as above; the model is not touched.  ``exclude`` is recommend()'s, by user id
    def recommend_users(self, sides, k: int, items=None, exclude=None, new_items=None, new_users=None):
        """The ``k`` (1..64) best users of ``sides`` per item: ``(users int32 [n, k], scores float64
        [n, k])``, ranked by logit (ties: higher user index first), scores as ``predict()`` gives
        them -- the score of (item i, user u) has the bytes ``recommend()`` gives (u, i); short
        lists are padded with user -1 / score NaN."""
        from . import recommend as rec

        return rec.topk_users(*rec.operands(self, sides, new_users=new_users, new_items=new_items), k, items, exclude)

    def rank_users(self, sides, items, users, exclude=None, new_items=None, new_users=None):
        """Where user ``users[n]`` stands among all users of ``sides`` in item ``items[n]``'s ranking:
        ``(ranks int32 [n], scores float64 [n], candidates int32 [n])`` in input order, ranks
        0-based under ``recommend_users()``'s order, at any depth (recommend.py)."""
        from . import recommend as rec

        return rec.rank_users(*rec.operands(self, sides, new_users=new_users, new_items=new_items), items, users,
                              exclude)

    def rank_audience(self, sides, depth: int, items=None, exclude=None, new_items=None, new_users=None,
                      workspace_bytes=None):
        """Every item's ranking of the users of ``sides`` down to ``depth`` (any integer >= 1):
        ``(users int32 [n, depth], scores float64 [n, depth], n_ranked int32 [n])`` under
        ``recommend_users()``'s order, short rows padded with user -1 / score NaN (recommend.py)."""
        from . import recommend as rec

        return rec.rank_audience(*rec.operands(self, sides, new_users=new_users, new_items=new_items), depth, items,
                                 exclude, workspace_bytes)

    # new_items / new_users: the FoldedColumns of the matching fold_in_* are the queries (their served
    # operand A) against the catalogue's own rows -- ``items`` / ``users`` then index the folded rows
    def similar_items(self, sides, k: int, items=None, metric="cosine", exclude=None, include_self=False,
                      new_items=None):
        """The ``k`` (1..64) items of ``sides`` most like each item: ``(items int32 [n, k], values
        float64 [n, k])``, the cosine (``metric="dot"``: the dot product) of the item vectors
        ``b_i = sum_j xi_j V[j,:]``, best first, ties: higher index first, an item never its own
        neighbour unless ``include_self``; ``exclude``: CSR by item id.  Similarity is in factor
        space only: ``w0``, ``w`` and the sides' own pair terms play no part.  An item without
        entries has no direction: it is nobody's neighbour and its list is empty (recommend.neighbours)."""
        from . import recommend as rec

        return rec.similar(self, "item", k, items, metric, exclude, include_self, new_items, sides)

    def similar_users(self, sides, k: int, users=None, metric="cosine", exclude=None, include_self=False,
                      new_users=None):
        """``similar_items`` for the user vectors ``a_u = sum_j xu_j V[j,:]`` of ``sides``, in factor
        space only."""
        from . import recommend as rec

        return rec.similar(self, "user", k, users, metric, exclude, include_self, new_users, sides)
