"""The per-iteration validation metric of ``fit(..., evaluator=)`` on the device
(SURVEY.md 8f N1).

The reference calls ``evaluator.evaluate(y_scores=predict(...), estimator=...)``
after every iteration (``src/fm.py:104-110``, ``src/mf.py:126-132``); for its
``ValEvaluator`` that is a pandas ``groupby("user")`` plus one ``argsort`` per
user on the host (``utils/evaluate.py:183-239``).  When the object handed in is
recognisably such an evaluator -- a frame ``interaction_df`` with the columns
``user, label, pscore, ones_pscore``, a ranking depth ``k`` and
``metric_name == "DCG"`` -- the same IPS-DCG@k is computed by ``rfm_val_dcg``
from the scores that are already in HBM, and only the list of metric values
comes back when ``fit`` ends.  Any other object keeps the host callback.

Ranking ties: the device ranks equal scores later-row-first
(``argsort(kind="stable")[::-1]``).  NumPy's default sort, which the reference
calls, is not stable and its tie order changes from CPU to CPU, and saturated
sigmoid scores (exactly 0.0 / 1.0) make ties common.  ``rfm_val_dcg`` therefore
flags the users whose value depends on the tie order; for exactly those users the
value is recomputed on the host the way the reference does it -- the same
``ndarray.argsort()[::-1]`` on the same per-user score array, the same formula
(``utils/metrics.py:53-80``) -- so ``val_metrics`` is what the host callback would
have produced on this machine, while the unambiguous users (the bulk) never leave
the device (``EvalLoop``).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib
from . import recommend as rec
from .runtime import Runtime

_COLUMNS = ("user", "label", "pscore", "ones_pscore")


def group_by_user(users: np.ndarray):
    """``(order, seg_ptr)``: frame rows grouped by ascending user, rows of a
    group in frame order (``groupby("user").agg(list)``, evaluate.py:225-239)."""
    users = np.asarray(users)
    n = users.shape[0]
    order = np.argsort(users, kind="stable").astype(np.int32)
    su = users[order]
    cuts = np.flatnonzero(su[1:] != su[:-1]) + 1
    seg_ptr = (np.concatenate(([0], cuts, [n])) if n else np.zeros(1)).astype(np.int32)
    return order, seg_ptr


class ValFrame:
    """A validation frame grouped by user, on the host: what the order-dependent users are
    redone from (and all that is needed to restate ``ValEvaluator.evaluate`` without a GPU)."""

    def __init__(self, users, labels, pscores: Optional[np.ndarray], k: int):
        users = np.asarray(users)
        if users.ndim != 1:
            raise ValueError("users must be a 1-D array")
        n = users.shape[0]
        if k < 1:
            raise ValueError("k (ranking positions) must be >= 1")
        self.k, self.n_rows = int(k), int(n)
        self.h_order, self.h_seg_ptr = group_by_user(users)
        self.n_segments = int(self.h_seg_ptr.shape[0] - 1)
        labels = np.asarray(labels, dtype=np.float64)
        if labels.shape != (n,):
            raise ValueError("labels must match the frame's rows")
        self.h_labels = labels[self.h_order] if n else np.zeros(0)
        self.h_pscores = None
        if pscores is not None:
            pscores = np.asarray(pscores, dtype=np.float64)
            if pscores.shape != (n,):
                raise ValueError("pscores must match the frame's rows")
            self.h_pscores = pscores[self.h_order] if n else np.zeros(0)

    def take_groups(self, lo: int, hi: int) -> "ValFrame":
        """User groups ``lo .. hi - 1`` as a frame of their own whose rows are theirs in grouped
        order: its row ``j`` is row ``h_order[h_seg_ptr[lo] + j]`` of this frame, its group ``g``
        is group ``lo + g`` here (a rank's shard of the log in ``dist.fit_data_parallel``)."""
        r0, r1 = int(self.h_seg_ptr[lo]), int(self.h_seg_ptr[hi])
        out = ValFrame.__new__(ValFrame)
        out.k, out.n_rows = self.k, r1 - r0
        out.h_order = np.arange(r1 - r0, dtype=np.int32)
        out.h_seg_ptr = (self.h_seg_ptr[lo: hi + 1] - r0).astype(np.int32)
        out.n_segments = int(hi - lo)
        out.h_labels = self.h_labels[r0:r1].copy()
        out.h_pscores = None if self.h_pscores is None else self.h_pscores[r0:r1].copy()
        return out

    def host_user_value(self, scores: np.ndarray, g: int) -> float:
        """IPS-DCG@k of user group ``g`` exactly as the reference computes it
        (utils/evaluate.py:194-204 with utils/metrics.py:53-80), including whatever order
        NumPy's default sort leaves equal scores in."""
        lo, hi = int(self.h_seg_ptr[g]), int(self.h_seg_ptr[g + 1])
        ranked = scores[self.h_order[lo:hi]].argsort()[::-1]
        y = self.h_labels[lo:hi][ranked]
        p = np.ones(hi - lo) if self.h_pscores is None else self.h_pscores[lo:hi][ranked]
        value = 0.0
        value += y[0] / p[0]
        tail = y[1:self.k]
        positions = np.arange(1, tail.shape[0] + 1)
        value += np.sum(tail / (p[1:self.k] * np.log2(positions + 1)))
        return float(value)

    def host_user_values(self, scores: np.ndarray, groups: np.ndarray) -> np.ndarray:
        """``host_user_value`` of many groups at once: groups of equal length are stacked and
        ranked by one ``argsort(axis=1)`` -- NumPy runs the same 1-D sort on every row, so each
        row gets the order (ties included) its own ``argsort()`` call would give."""
        out = np.empty(groups.shape[0], dtype=np.float64)
        lo = self.h_seg_ptr[groups].astype(np.int64)
        lens = self.h_seg_ptr[groups + 1].astype(np.int64) - lo
        for length in np.unique(lens):
            sel = np.flatnonzero(lens == length)
            idx = lo[sel][:, None] + np.arange(length)[None, :]
            ranked = np.argsort(scores[self.h_order[idx]], axis=1)[:, ::-1]
            y = np.take_along_axis(self.h_labels[idx], ranked, axis=1)
            p = (np.ones_like(y) if self.h_pscores is None
                 else np.take_along_axis(self.h_pscores[idx], ranked, axis=1))
            value = 0.0 + y[:, 0] / p[:, 0]
            tail = y[:, 1:self.k]
            positions = np.arange(1, tail.shape[1] + 1)
            value = value + np.sum(tail / (p[:, 1:self.k] * np.log2(positions + 1)[None, :]), axis=1)
            out[sel] = value
        return out

    def resolve(self, scores: np.ndarray, user_scratch: np.ndarray) -> float:
        """The metric from the device's per-user results (``user_scratch`` = the
        ``3 * n_segments`` doubles of one ``rfm_val_dcg``) with the order-dependent users
        recomputed the reference's way on the host."""
        n = self.n_segments
        vals = user_scratch[:n].copy()
        counted = user_scratch[n: 2 * n] != 0.0
        redo = np.flatnonzero(user_scratch[2 * n: 3 * n] != 0.0)
        if redo.size:
            vals[redo] = self.host_user_values(scores, redo)
        return float(np.mean(vals[counted]))


class DeviceValFrame(ValFrame):
    """The grouped frame resident in HBM."""

    def __init__(self, rt: Runtime, users, labels, pscores: Optional[np.ndarray], k: int):
        super().__init__(users, labels, pscores, k)
        self.rt = rt
        n = self.n_rows
        self.rows = rt.upload(self.h_order if n else np.zeros(1, np.int32))
        self.seg_ptr = rt.upload(self.h_seg_ptr)
        self.labels = rt.upload(self.h_labels if n else np.zeros(1))
        self.pscores = None
        if self.h_pscores is not None:
            self.pscores = rt.upload(self.h_pscores if n else np.zeros(1))
        self.scratch = rt.empty((max(3 * self.n_segments, 1),), self.labels.dtype)

    def dcg_into(self, d_scores, out_ptr: int, scratch_ptr: Optional[int] = None) -> None:
        """Enqueue the metric of ``d_scores`` (device, frame order): the value and the
        number of users it is tie-order dependent for land at ``out_ptr`` (2 doubles), the
        per-user values / counted / order-dependent flags in ``3 * n_segments`` doubles at
        ``scratch_ptr`` (default: this frame's own scratch)."""
        rt = self.rt
        _lib.check(rt.lib.rfm_val_dcg(
            rt.ctx, d_scores.data_ptr(), self.seg_ptr.data_ptr(), self.rows.data_ptr(),
            self.labels.data_ptr(), None if self.pscores is None else self.pscores.data_ptr(),
            self.n_segments, self.k, self.scratch.data_ptr() if scratch_ptr is None else scratch_ptr,
            out_ptr))

    def dcg_checked(self, scores):
        """``(value, n_order_dependent_users)`` of host or device scores (frame order)."""
        rt = self.rt
        d = scores if hasattr(scores, "data_ptr") else rt.upload(np.asarray(scores, dtype=np.float64))
        if d.shape[0] != self.n_rows:
            raise ValueError(f"{d.shape[0]} scores for a frame of {self.n_rows} rows")
        out = rt.empty((2,), self.labels.dtype)
        self.dcg_into(d, out.data_ptr())
        rt.sync()
        o = out.cpu().numpy()
        return float(o[0]), int(o[1])

    def dcg(self, scores) -> float:
        """The metric under the device's tie rule, synchronously."""
        return self.dcg_checked(scores)[0]

    def per_user(self):
        """``(values, counted, order_dependent)`` of the last call, one entry per user group."""
        self.rt.sync()
        s = self.scratch.cpu().numpy()
        n = self.n_segments
        return s[:n].copy(), s[n: 2 * n] != 0.0, s[2 * n: 3 * n] != 0.0


def runs(first: int, count: int, limit):
    """``(at, n)`` of consecutive runs that cover iterations ``first .. first + count``, the run
    that starts at ``at`` no longer than ``limit(at)``: how every fit cuts an id chunk into
    library calls."""
    at, end = first, first + count
    while at < end:
        n = min(end - at, limit(at))
        yield at, n
        at += n


def leave_y_score(evaluator, y_scores: np.ndarray) -> None:
    """The reference's ``evaluate`` stores the scores it was given in its frame
    (``interaction_df["y_score"] = y_scores``, utils/evaluate.py:224): so does a fit that never
    called it."""
    try:
        evaluator.interaction_df["y_score"] = y_scores
    except Exception:  # noqa: BLE001 -- a read-only or exotic frame: nothing to leave
        pass


class SlotLoop:
    """Chunks of per-iteration score slots on the device and the metric list they become: what
    ``EvalLoop`` and ``dist.DpEvalLoop`` share.  ``out [n_epochs, 2]`` receives every iteration's
    value and the number of users it is tie-order dependent for; nothing returns to the host until
    a chunk of iterations is complete (``_flush``), and the flagged iterations of a chunk are then
    resolved by one ``_resolve`` call of the subclass."""

    def __init__(self, rt: Runtime, n_epochs: int, per_iter_bytes: int):
        self.rt, self.n_epochs = rt, n_epochs
        self.chunk = int(max(1, min(max(n_epochs, 1), EvalLoop.CHUNK_BYTES // per_iter_bytes)))
        self.out = rt.empty((max(n_epochs, 1), 2), __import__("torch").float64)
        self.values: list = []
        self.host_calls = 0   # iterations that needed host work
        self.host_users = 0   # users redone on the host, over all iterations
        self._flushed = 0

    def room(self, epoch: int) -> int:
        """Iterations from ``epoch`` on that fit the current chunk of score slots."""
        return self.chunk - epoch % self.chunk

    def ran(self, first: int, count: int) -> None:
        """Iterations ``first .. first + count`` (inside one chunk: ``count <= room(first)``) were
        scored and measured."""
        if (first + count) % self.chunk == 0:
            self._flush(first + count)

    def _resolve(self, flagged: list) -> dict:
        """``{iteration: value}`` of the iterations with tie-order dependent users."""
        raise NotImplementedError

    def _flush(self, upto: int) -> None:
        if upto <= self._flushed:
            return
        self.rt.sync()
        o = self.out[self._flushed:upto].cpu().numpy()
        epochs = range(self._flushed, upto)
        fixed = self._resolve([e for i, e in enumerate(epochs) if o[i, 1] != 0.0])
        for i, e in enumerate(epochs):
            if e in fixed:
                self.values.append(fixed[e])
                self.host_calls += 1
                self.host_users += int(o[i, 1])
            else:
                self.values.append(float(o[i, 0]))
        self._flushed = upto

    def finish(self, n_done: int) -> list:
        self._flush(n_done)
        return self.values


class EvalLoop(SlotLoop):
    """The evaluator hook of a ``fit()`` loop, computed on the device.

    Per iteration the caller writes the evaluator's scores into ``slot(epoch)`` and calls
    ``measure(epoch)`` (MF), or the library does both (``rfm_fm_train_eval`` with ``call_args``);
    either way ``ran`` follows.  For an iteration with tie-order dependent users, the scores
    and the per-user results come back and those users are redone the reference's way
    (``DeviceValFrame.resolve``) -- the list ``finish()`` returns is what calling the
    evaluator every iteration would have produced on this machine.  ``log``: the evaluator's
    features on the device -- FM's matrix (``call_args``), MF's pairs."""

    CHUNK_BYTES = 1 << 30

    def __init__(self, rt: Runtime, frame: DeviceValFrame, evaluator, estimator: str, n_epochs: int, log=None):
        super().__init__(rt, n_epochs, 8 * (frame.n_rows + 3 * frame.n_segments) + 8)
        self.frame, self.evaluator, self.estimator, self.log = frame, evaluator, estimator, log
        self.scores = rt.empty((self.chunk, max(frame.n_rows, 1)), frame.labels.dtype)
        self.users = rt.empty((self.chunk, max(3 * frame.n_segments, 1)), frame.labels.dtype)

    def slot(self, epoch: int):
        """Device tensor the scores of iteration ``epoch`` go to."""
        return self.scores[epoch % self.chunk]

    def measure(self, epoch: int) -> None:
        """Enqueue the metric of the scores in ``slot(epoch)``; the caller then reports ``ran(epoch, 1)``."""
        self.frame.dcg_into(self.slot(epoch), self.out.data_ptr() + epoch * 16,
                            self.users[epoch % self.chunk].data_ptr())

    def call_args(self, first: int) -> tuple:
        """The evaluation arguments of ``rfm_fm_train_eval`` for a run that starts at ``first``."""
        ev, fr = self.log, self.frame
        return (ev.indptr.data_ptr(), ev.indices.data_ptr(), ev.values.data_ptr(), ev.shape[0],
                fr.seg_ptr.data_ptr(), fr.rows.data_ptr(), fr.labels.data_ptr(),
                None if fr.pscores is None else fr.pscores.data_ptr(), fr.n_segments, fr.k,
                self.scores.data_ptr(), self.scores.shape[1], self.users.data_ptr(), self.users.shape[1],
                first % self.chunk, self.out.data_ptr() + first * 16)

    def _resolve(self, flagged: list) -> dict:
        return {e: self.frame.resolve(self.slot(e)[: self.frame.n_rows].cpu().numpy(),
                                      self.users[e % self.chunk].cpu().numpy()) for e in flagged}

    def leave_scores(self, epoch: int) -> None:
        """The last iteration's scores into the evaluator's frame, as the last host callback
        would have left them (``leave_y_score``)."""
        if epoch < 0:
            return
        self.rt.sync()
        leave_y_score(self.evaluator, self.slot(epoch)[: self.frame.n_rows].cpu().numpy())


def known_implementation(evaluator) -> bool:
    """True when ``evaluator.evaluate`` is known to be the reference's IPS-DCG@k: the class
    that DEFINES ``evaluate`` is ``ValEvaluator`` of a module called ``evaluate``
    (``utils/evaluate.py:160-207``; a subclass that overrides ``evaluate()`` is not), or the
    object opts in with ``rfm_device_evaluator = True``."""
    if getattr(evaluator, "rfm_device_evaluator", False) is True:
        return True
    for cls in type(evaluator).__mro__:
        if "evaluate" in vars(cls):
            return cls.__qualname__ == "ValEvaluator" and cls.__module__.split(".")[-1] == "evaluate"
    return False


def recognise(evaluator, estimator: str, any_implementation: bool = False):
    """``(users, labels, pscores, k)`` of the reference's ValEvaluator (or an object that
    opts in, see ``known_implementation``), or ``None`` when it is something else (then the
    caller keeps the host callback).  ``any_implementation`` skips the check of whose
    ``evaluate()`` it is and looks at the attributes only."""
    if not any_implementation and not known_implementation(evaluator):
        return None
    frame = getattr(evaluator, "interaction_df", None)
    k = getattr(evaluator, "k", None)
    if frame is None or not isinstance(k, (int, np.integer)) or k < 1:
        return None
    if getattr(evaluator, "metric_name", None) != "DCG":
        return None
    try:
        cols = {c: np.asarray(frame[c]) for c in _COLUMNS}
    except (KeyError, TypeError, IndexError, ValueError):
        return None
    n = cols["user"].shape[0]
    if any(v.ndim != 1 or v.shape[0] != n for v in cols.values()):
        return None
    # evaluate.py:222: pscore for IPS, ones_pscore for every other estimator
    p = cols["pscore"] if estimator == "IPS" else cols["ones_pscore"]
    return cols["user"], cols["label"], p, int(k)


def host_frame(evaluator, estimator: str, n_scores: int) -> Optional[ValFrame]:
    """The grouped host frame of ``evaluator`` under the rule of ``device_frame`` (recognised, and
    ``n_scores`` rows); else ``None``."""
    got = recognise(evaluator, estimator)
    if got is None or got[0].shape[0] != n_scores:
        return None
    users, labels, pscores, k = got
    return ValFrame(users, labels, pscores, k)


def device_frame(rt: Runtime, evaluator, estimator: str, n_scores: int) -> Optional[DeviceValFrame]:
    """The device form of ``evaluator`` if it is recognised and matches the
    ``n_scores`` rows its features produce; else ``None``."""
    got = recognise(evaluator, estimator)
    if got is None or got[0].shape[0] != n_scores:
        return None
    users, labels, pscores, k = got
    return DeviceValFrame(rt, users, labels, pscores, k)


class FitHook:
    """What one fit does about ``model.evaluator``: the one place where its path is chosen, for
    ``FactorizationMachines.fit``, ``LogisticMatrixFactorization.fit`` and
    ``dist.fit_data_parallel``.

    - ``cat``: a ``CatalogueValEvaluator`` is given the model and enqueues its own evaluations
      (DESIGN.md 8 N8);
    - ``loop``: with ``model.device_evaluator``, ``make_loop(evaluator)`` -- the driver's score-slot
      loop (``EvalLoop``, ``dist.DpEvalLoop``) -- or ``None`` when the driver has no device path
      (``make_loop=None``) or does not recognise the evaluator (``device_frame`` / ``host_frame``);
    - otherwise an evaluator is a host callback after every iteration, on ``predict``'s scores.

    The driver cuts its id chunks with ``runs(first, count, hook.limit)``, calls ``ran`` after
    enqueueing each run and ``finish`` once the stream is idle."""

    def __init__(self, model, n_epochs: int, predict, make_loop=None):
        self.model, self.n_epochs, self.predict = model, n_epochs, predict
        self.evaluator = getattr(model, "evaluator", None)
        self.cat = self.loop = None
        if isinstance(self.evaluator, CatalogueValEvaluator):
            self.cat = self.evaluator
            self.cat.fit_begin(model, n_epochs)
        elif self.evaluator is not None and make_loop is not None and getattr(model, "device_evaluator", False):
            self.loop = make_loop(self.evaluator)

    def limit(self, at: int) -> int:
        """How many iterations the run that starts at ``at`` may hold."""
        if self.cat is not None:
            return self.cat.fit_run_length(at)  # (ends at the next evaluation point)
        if self.loop is not None:
            return self.loop.room(at)
        return self.n_epochs if self.evaluator is None else 1

    def ran(self, at: int, n: int) -> None:
        """Iterations ``at .. at + n`` were enqueued."""
        last = at + n - 1
        if self.cat is not None:
            if self.cat.fit_due(last):
                self.cat.fit_enqueue(last)  # (behind the iteration, on the same stream)
        elif self.loop is not None:
            self.loop.ran(at, n)
        elif self.evaluator is not None:
            m = self.model
            y_scores = self.predict(self.evaluator.features[m.model_name])
            m.val_metrics.append(self.evaluator.evaluate(y_scores=y_scores, estimator=m.estimator))

    def finish(self) -> None:
        """The metric list into ``model.val_metrics``; the device loop's counters and last scores."""
        m = self.model
        if self.cat is not None:
            m.val_metrics.extend(self.cat.fit_end())
        elif self.loop is not None:
            m.val_metrics.extend(self.loop.finish(self.n_epochs))
            m.evaluator_host_calls = self.loop.host_calls
            m.evaluator_host_users = self.loop.host_users
            self.loop.leave_scores(self.n_epochs - 1)


# ---------------------------------------------------------------------------
# test-set metrics: TestEvaluator on device-ranked rows
# ---------------------------------------------------------------------------
TEST_METRICS = ("Recall", "MAP", "DCG", "ME", "CatalogCoverage", "Gini")  # utils/metrics.py:169-178


class TestFrame:
    """A test frame grouped by user and the metrics of ``TestEvaluator.evaluate``
    (``utils/evaluate.py:80-127``) from the positions of every user's best ``max(K)`` rows.
    Host only: the ranking is what the device does (``DeviceTestEvaluator``); the metrics
    themselves are sums over ``n_users x max(K)`` values."""

    __test__ = False  # not a pytest class

    def __init__(self, users, items, labels, pscores, K, used_metrics, n_items: int):
        self.K = tuple(int(k) for k in K)
        if not self.K or min(self.K) < 1:
            raise ValueError("K (ranking positions) must be positive")
        self.kmax = max(self.K)
        # the reference always reports ME, then the metrics it was asked for (evaluate.py:66-78)
        self.names = ["ME"]
        for name in used_metrics:
            if name not in TEST_METRICS:
                raise ValueError(f"metric_name must be in {TEST_METRICS}. metric_name: '{name}'")
            if name not in self.names:
                self.names.append(name)
        self.n_items = int(n_items)
        users = np.asarray(users)
        n = users.shape[0]
        self.n_rows = int(n)
        self.h_order, self.h_seg_ptr = group_by_user(users)
        self.n_segments = int(self.h_seg_ptr.shape[0] - 1)
        cols = []
        for arr, dt in ((labels, np.float64), (pscores, np.float64), (items, np.int64)):
            arr = np.asarray(arr, dtype=dt)
            if arr.shape != (n,):
                raise ValueError("frame columns must match its rows")
            cols.append(arr[self.h_order] if n else arr)
        self.h_labels, self.h_pscores, self.h_items = cols
        self.h_ysum = (np.add.reduceat(self.h_labels, self.h_seg_ptr[:-1].astype(np.int64))
                       if n else np.zeros(0))

    def host_topk(self, scores: np.ndarray, g: int) -> np.ndarray:
        """Positions of user ``g``'s best rows exactly as the reference ranks them
        (``argsort()[::-1]``, whatever order NumPy leaves equal scores in)."""
        lo, hi = int(self.h_seg_ptr[g]), int(self.h_seg_ptr[g + 1])
        ranked = scores[self.h_order[lo:hi]].argsort()[::-1][: self.kmax]
        out = np.full(self.kmax, -1, dtype=np.int64)
        out[: ranked.shape[0]] = lo + ranked
        return out

    def metrics(self, pos: np.ndarray, flags: np.ndarray, scores: np.ndarray) -> dict:
        """``{metric: [value per K]}`` from the device's ``pos [n_users][kmax]`` / ``flags``
        (``rfm_topk_users``); users flagged order-dependent are ranked again on the host."""
        pos = np.asarray(pos, dtype=np.int64).reshape(self.n_segments, self.kmax).copy()
        flags = np.asarray(flags)
        for g in np.flatnonzero(flags & 2):
            pos[g] = self.host_topk(scores, int(g))
        counted = np.flatnonzero(flags & 1)
        P = pos[counted]
        valid = P >= 0
        safe = np.where(valid, P, 0)
        Y = np.where(valid, self.h_labels[safe] if self.n_rows else 0.0, 0.0)
        PS = np.where(valid, self.h_pscores[safe] if self.n_rows else 0.0, np.nan)
        IT = np.where(valid, self.h_items[safe] if self.n_rows else 0, -1)
        ysum = self.h_ysum[counted] if self.n_rows else np.zeros(0)
        out = {}
        with np.errstate(invalid="ignore", divide="ignore"):
            for name in self.names:
                vals = []
                for k in self.K:
                    if name == "ME":  # utils/metrics.py:110-126
                        vals.append(_nanmean(PS[:, k - 1]))
                    elif name == "DCG":  # utils/metrics.py:83-107
                        disc = np.log2(np.arange(1, k) + 1)
                        vals.append(_nanmean(0.0 + Y[:, 0] + np.sum(Y[:, 1:k] / disc[None, :], axis=1)))
                    elif name == "Recall":  # utils/metrics.py:32-50
                        vals.append(_nanmean(np.sum(Y[:, :k], axis=1) / ysum))
                    elif name == "MAP":  # utils/metrics.py:9-29
                        hits = (Y[:, :k] >= 1) & valid[:, :k]
                        prec = np.cumsum(Y[:, :k], axis=1) / np.arange(1, k + 1)[None, :]
                        vals.append(_nanmean(np.sum(np.where(hits, prec, 0.0), axis=1)))
                    elif name == "CatalogCoverage":  # utils/metrics.py:151-166
                        rec = IT[:, :k][valid[:, :k]]
                        vals.append(len(np.unique(rec)) / self.n_items)
                    else:  # Gini, utils/metrics.py:129-148
                        rec = IT[:, :k][valid[:, :k]]
                        rec = rec[(rec >= 0) & (rec < self.n_items)]
                        freqs = np.sort(np.bincount(rec, minlength=self.n_items), kind="merge")
                        idx = np.arange(1, self.n_items + 1)
                        vals.append(float(np.sum((2 * idx - self.n_items - 1) * freqs)
                                          / (self.n_items * np.sum(freqs))))
                out[name] = vals
        return out


def _nanmean(a: np.ndarray) -> float:
    import warnings

    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)  # mean of no users is nan
        return float(np.nanmean(a)) if a.size else float("nan")


class DeviceTestEvaluator:
    """``TestEvaluator`` (``utils/evaluate.py:42-156``) with the per-user ranking on the
    device: same constructor fields (``interaction_df`` with the columns user / item / label /
    pscore, ``features``, ``K``, ``used_metrics``, ``n_items``), same ``evaluate(y_scores)``
    result -- ``{metric: [value per K]}`` with ``ME`` always present -- and the same side
    effect (``interaction_df["y_score"]``)."""

    def __init__(self, interaction_df, features, K, used_metrics, n_items: int, rt: Optional[Runtime] = None):
        from collections import defaultdict

        self.interaction_df, self.features = interaction_df, features
        self.K, self.used_metrics, self.n_items = K, used_metrics, n_items
        self._defaultdict = defaultdict
        self.rt = rt or Runtime.get()
        df = interaction_df
        self.frame = TestFrame(df["user"], df["item"], df["label"], df["pscore"], K, used_metrics, n_items)
        fr, up = self.frame, self.rt.upload
        n = fr.n_rows
        self._rows = up(fr.h_order if n else np.zeros(1, np.int32))
        self._seg = up(fr.h_seg_ptr)
        self._labels = up(fr.h_labels if n else np.zeros(1))
        self._pscores = up(fr.h_pscores if n else np.zeros(1))
        self._items = up((fr.h_items if n else np.zeros(1)).astype(np.int32))
        self.host_users = 0  # users ranked again on the host in the last evaluate()

    def topk(self, y_scores):
        """``(pos [n_users][max K], flags [n_users])`` of host or device scores (frame order)."""
        torch = __import__("torch")
        rt, fr = self.rt, self.frame
        d = y_scores if hasattr(y_scores, "data_ptr") else rt.upload(np.asarray(y_scores, dtype=np.float64))
        if d.shape[0] != fr.n_rows:
            raise ValueError(f"{d.shape[0]} scores for a frame of {fr.n_rows} rows")
        pos = rt.empty((max(fr.n_segments, 1), fr.kmax), torch.int32)
        flags = rt.empty((max(fr.n_segments, 1),), torch.int32)
        _lib.check(rt.lib.rfm_topk_users(
            rt.ctx, d.data_ptr(), self._seg.data_ptr(), self._rows.data_ptr(), self._labels.data_ptr(),
            self._pscores.data_ptr(), self._items.data_ptr(), fr.n_segments, fr.kmax, pos.data_ptr(),
            flags.data_ptr()))
        rt.sync()
        return pos.cpu().numpy()[: fr.n_segments], flags.cpu().numpy()[: fr.n_segments]

    def evaluate(self, y_scores):
        host_scores = y_scores.cpu().numpy() if hasattr(y_scores, "data_ptr") else np.asarray(y_scores, dtype=np.float64)
        pos, flags = self.topk(y_scores)
        self.host_users = int(np.count_nonzero(flags & 2))
        try:
            self.interaction_df["y_score"] = host_scores  # utils/evaluate.py:141
        except Exception:  # noqa: BLE001 -- a read-only frame
            pass
        results = self._defaultdict(list)
        for name, vals in self.frame.metrics(pos, flags, host_scores).items():
            results[name] = list(vals)
        return results


class CatalogueEvaluator:
    """Held-out interactions ranked against the WHOLE catalogue, where
    ``TestEvaluator`` ranks only the rows of the test log: every positive's position among all
    items its user could be shown, from ``model.rank_items`` (one call), and from the ranks on
    the host the reference's ``calc_dcg_at_k`` / ``calc_recall_at_k`` /
    ``calc_average_precision_at_k`` (``utils/metrics.py:9-107``) as they come out for the 0/1
    vector of the user's candidates in catalogue order, plus MRR and AUC.

    ``positives``: ``(users, items)`` of the held-out interactions (repeats are dropped);
    ``K``: ranking depths, any positive integers; ``used_metrics``: a subset of ``METRICS``;
    ``exclude``: items never shown to a user (the train pairs), as ``recommend()`` takes them --
    a positive that it lists is a ``ValueError`` of ``evaluate``.  ``evaluate`` returns
    ``{metric: [value per K]}`` (MRR, AUC: one value): the nan-mean over the users that have a
    ranked positive.  A positive of rank -1 (NaN logit) is left out and counted in ``unranked``."""

    METRICS = ("DCG", "Recall", "MAP", "MRR", "AUC")

    def __init__(self, positives, n_items: int, K, used_metrics, exclude=None):
        users, items = (np.asarray(a) for a in positives)
        if users.ndim != 1 or users.shape != items.shape:
            raise ValueError("positives must be two 1-d arrays of equal length: users, items")
        for a in (users, items):
            if a.size and not np.issubdtype(a.dtype, np.integer):
                raise ValueError("positives must be integer ids")
        self.n_items = int(n_items)
        if items.size and (items.min() < 0 or items.max() >= self.n_items):
            raise ValueError(f"an item id lies outside 0..{self.n_items - 1}")
        self.K = [int(k) for k in K]
        if any(k < 1 for k in self.K):
            raise ValueError("K must be positive integers")
        unknown = [m for m in used_metrics if m not in self.METRICS]
        if unknown:
            raise ValueError(f"unknown metric {unknown[0]!r} (known: {', '.join(self.METRICS)})")
        self.used_metrics = list(used_metrics)
        keys = np.unique(users.astype(np.int64) * self.n_items + items.astype(np.int64))
        self.users, self.items = keys // self.n_items, keys % self.n_items
        self.exclude = exclude
        self.unranked = 0  # positives without a rank in the last evaluate() / metrics()

    def metrics(self, users, ranks, candidates) -> dict:
        """The metrics from ``(user, rank, candidate count of the user)`` per positive: host only."""
        users, ranks, candidates = np.asarray(users), np.asarray(ranks).astype(np.int64), np.asarray(candidates)
        ranked = ranks >= 0
        self.unranked = int(np.count_nonzero(~ranked))
        users, ranks, candidates = users[ranked], ranks[ranked], candidates[ranked]
        order = np.lexsort((ranks, users))
        _, seg_ptr = group_by_user(users[order])
        per_user = {m: [] for m in self.used_metrics}
        for g in range(seg_ptr.shape[0] - 1):
            rows = order[seg_ptr[g]:seg_ptr[g + 1]]
            if rows.size == 0:
                continue
            r = ranks[rows].astype(np.float64)      # ascending: r_1 < ... < r_P
            P, C = r.shape[0], float(candidates[rows[0]])
            j = np.arange(1, P + 1, dtype=np.float64)
            gain = np.where(r == 0, 1.0, 1.0 / np.log2(np.maximum(r, 1.0) + 1.0))
            for m in self.used_metrics:
                if m == "DCG":
                    per_user[m].append([float(np.sum(gain[r < k])) for k in self.K])
                elif m == "Recall":
                    per_user[m].append([np.count_nonzero(r < k) / P for k in self.K])
                elif m == "MAP":
                    per_user[m].append([float(np.sum((j / (r + 1.0))[r < k])) for k in self.K])
                elif m == "MRR":
                    per_user[m].append([1.0 / (r[0] + 1.0)])
                elif m == "AUC":
                    per_user[m].append([1.0 - float(np.sum(r - (j - 1.0))) / (P * (C - P)) if C > P else np.nan])
        out = {}
        for m in self.used_metrics:
            width = 1 if m in ("MRR", "AUC") else len(self.K)
            vals = np.asarray(per_user[m], dtype=np.float64).reshape(-1, width)
            out[m] = [_nanmean(vals[:, c]) for c in range(width)]
        return out

    def evaluate(self, model, sides=None) -> dict:
        """``model``: a ``FactorizationMachines`` (with its ``recommend.Sides``) or a fitted
        ``LogisticMatrixFactorization``."""
        args = (self.users, self.items, self.exclude)
        ranks, _, candidates = model.rank_items(*args) if sides is None else model.rank_items(sides, *args)
        return self.metrics(self.users, ranks, candidates)


class CatalogueExposure:
    """The reference's three qualitative metrics -- mean exposure, catalogue coverage and Gini
    (``utils/metrics.py:110-166``, as ``TestEvaluator`` sums them, ``utils/evaluate.py:93-125``) --
    of every selected user's ranking of the WHOLE catalogue, from one
    ``model.rank_catalogue(depth=max(K))`` call.

    ``K``: ranking depths, any positive integers; ``used_metrics``: a subset of ``METRICS``;
    ``item_pscores [n_items]``: the propensity of an item, required by ``"ME"`` (in the reference
    the KuaiRec propensity is a function of the item, ``utils/dataloader/kuairec/_click.py:170-204``);
    ``exclude``: items never shown to a user, as ``recommend()`` takes them; ``users``: the users
    that count (default: all) -- there are no labels here, so ``TestEvaluator``'s "users with a
    positive" is the caller's choice.  ``evaluate`` returns ``{metric: [value per K]}``:
    ``CatalogCoverage@k`` = distinct items in the lists' first k columns / ``n_items``, ``Gini@k``
    = ``calc_gini_at_k`` over the same items, ``ME@k`` = nan-mean over the users of the propensity
    of the item at position k - 1 (NaN for a user with fewer than k ranked items)."""

    METRICS = ("ME", "CatalogCoverage", "Gini")

    def __init__(self, n_items: int, K, used_metrics, item_pscores=None, exclude=None, users=None):
        self.n_items = int(n_items)
        self.K = [int(k) for k in K]
        if not self.K or any(k < 1 for k in self.K):
            raise ValueError("K must be positive integers")
        unknown = [m for m in used_metrics if m not in self.METRICS]
        if unknown:
            raise ValueError(f"unknown metric {unknown[0]!r} (known: {', '.join(self.METRICS)})")
        self.used_metrics = list(used_metrics)
        self.item_pscores = None if item_pscores is None else np.asarray(item_pscores, dtype=np.float64)
        if "ME" in self.used_metrics and self.item_pscores is None:
            raise ValueError("'ME' needs item_pscores: the propensity of every item")
        if self.item_pscores is not None and self.item_pscores.shape != (self.n_items,):
            raise ValueError(f"item_pscores has shape {self.item_pscores.shape}, expected {(self.n_items,)}")
        self.exclude, self.users = exclude, users

    def metrics(self, items) -> dict:
        """The metrics from the lists ``items [n_users, depth]`` (-1 = no item): host only.  Columns
        past ``depth`` count as padding."""
        items = np.asarray(items).astype(np.int64)
        if items.ndim != 2:
            raise ValueError("items must be [n_users, depth]")
        kmax = max(self.K)
        if items.shape[1] < kmax:
            items = np.hstack([items, np.full((items.shape[0], kmax - items.shape[1]), -1, dtype=np.int64)])
        valid = items >= 0
        idx = np.arange(1, self.n_items + 1)
        out = {}
        for name in self.used_metrics:
            vals = []
            for k in self.K:
                if name == "ME":  # utils/metrics.py:110-126
                    col = items[:, k - 1]
                    vals.append(_nanmean(np.where(col >= 0, self.item_pscores[np.maximum(col, 0)], np.nan)))
                    continue
                rec = items[:, :k][valid[:, :k]]
                rec = rec[rec < self.n_items]
                if name == "CatalogCoverage":  # utils/metrics.py:151-166
                    vals.append(len(np.unique(rec)) / self.n_items)
                else:  # Gini, utils/metrics.py:129-148
                    freqs = np.sort(np.bincount(rec, minlength=self.n_items), kind="merge")
                    with np.errstate(invalid="ignore", divide="ignore"):
                        vals.append(float(np.sum((2 * idx - self.n_items - 1) * freqs) / (self.n_items * np.sum(freqs))))
            out[name] = vals
        return out

    def evaluate(self, model, sides=None) -> dict:
        """``model``: a ``FactorizationMachines`` (with its ``recommend.Sides``) or a fitted
        ``LogisticMatrixFactorization``."""
        args = (max(self.K), self.users, self.exclude)
        items, _, _ = model.rank_catalogue(*args) if sides is None else model.rank_catalogue(sides, *args)
        return self.metrics(items)


class CatalogueValEvaluator:
    """``CatalogueEvaluator``'s metrics per iteration of a ``fit()``: given as
    ``evaluator=`` to ``FactorizationMachines`` / ``LogisticMatrixFactorization``, it fills
    ``model.val_metrics`` with one column of the catalogue metrics -- the curve the reference's
    hyper-parameter search takes ``argmax`` of -- computed on the device from the model's
    parameters (side sums, ``rfm_pair_ranks_n``, ``rfm_rank_metrics``) with nothing coming back to
    the host before the fit ends.  ``evaluate(model)`` is the same evaluation, one-shot.

    ``positives``, ``n_items``, ``K`` (1 to 16 depths), ``used_metrics``, ``exclude``: as
    ``CatalogueEvaluator`` takes them, a positive that ``exclude`` names is a ``ValueError`` here.
    ``monitor``: ``(metric, k)``, the column that goes to ``val_metrics`` (``("MRR", None)``,
    ``("AUC", None)`` for the two without a depth).  ``sides``: the model's ``recommend.Sides`` for
    FM, None for MF.  ``pscores``: one propensity per positive, in input order; under the estimator
    ``"IPS"`` DCG@K becomes the reference's ``calc_ips_of_dcg_at_k`` (``utils/metrics.py:53-80``:
    every positive's gain divided by its propensity), every other estimator uses ones
    (``utils/evaluate.py:223``) and every other metric has no propensity-weighted form in the
    reference.  ``every``: evaluate after iteration e (0-based) when ``(e + 1) % every == 0``, and
    after the last one.

    After a fit: ``history = {metric: ndarray [n_epochs, width]}`` and ``unranked_history int64
    [n_epochs]``, NaN / -1 in the rows of iterations that were not evaluated."""

    METRICS = CatalogueEvaluator.METRICS
    MAX_DEPTHS = 16

    def __init__(self, positives, n_items: int, K, used_metrics, monitor, sides=None, exclude=None,
                 pscores=None, every: int = 1):
        base = CatalogueEvaluator(positives, n_items, K, used_metrics, exclude)  # (its checks)
        self.n_items, self.K, self.used_metrics, self.exclude = base.n_items, base.K, base.used_metrics, exclude
        if not 1 <= len(self.K) <= self.MAX_DEPTHS:
            raise ValueError(f"K must hold 1 to {self.MAX_DEPTHS} depths, got {len(self.K)}")
        users, items = (np.asarray(a).astype(np.int64) for a in positives)
        if users.size and users.min() < 0:
            raise ValueError("a user id is negative")
        keys, first, inverse = np.unique(users * self.n_items + items, return_index=True, return_inverse=True)
        self.users, self.items = keys // self.n_items, keys % self.n_items
        self.pscores = None
        if pscores is not None:
            ps = np.asarray(pscores, dtype=np.float64)
            if ps.shape != users.shape:
                raise ValueError(f"{ps.shape[0] if ps.ndim == 1 else ps.shape} pscores for {users.shape[0]} positives")
            if ps.size and not (np.isfinite(ps).all() and ps.min() > 0.0):
                raise ValueError("pscores must be positive and finite")
            self.pscores = ps[first]
            if np.any(ps != self.pscores[inverse.reshape(-1)]):
                raise ValueError("a repeated positive carries two different pscores")
        try:
            metric, depth = monitor
        except (TypeError, ValueError):
            raise ValueError("monitor must be (metric, k)") from None
        if metric not in self.used_metrics:
            raise ValueError(f"monitor: {metric!r} is not among used_metrics {self.used_metrics}")
        if metric in ("MRR", "AUC"):
            if depth is not None:
                raise ValueError(f"monitor: {metric} has no depth, use ({metric!r}, None)")
            self._monitor = (metric, 0)
        else:
            if not rec.is_int(depth) or int(depth) not in self.K:
                raise ValueError(f"monitor: depth {depth!r} is not among K {self.K}")
            self._monitor = (metric, self.K.index(int(depth)))
        self.monitor = (metric, depth)
        if not rec.is_int(every) or every < 1:
            raise ValueError(f"every must be an integer >= 1, got {every!r}")
        self.every = int(every)
        if sides is not None and not isinstance(sides, rec.Sides):
            raise ValueError("sides must be a recommend.Sides (FM) or None (MF)")
        self.sides = sides
        self._excl = None
        if exclude is not None:
            n_rows = (len(exclude[0]) - 1) if isinstance(exclude, (tuple, list)) else exclude.shape[0]
            self._excl = rec._host_exclusions(exclude, int(n_rows), self.n_items)
            p = rec._first_excluded_pair(self.users, self.items, self._excl, self.n_items)
            if p is not None:
                raise ValueError(f"positive (user {int(self.users[p])}, item {int(self.items[p])}) is in the "
                                 f"user's exclusion list: it has no rank")
        # the targets as rfm_pair_ranks takes them: the keys are sorted by (user, item)
        self._sel, self._indptr = rec.users_indptr(self.users)
        self._h_K = np.ascontiguousarray(self.K, dtype=np.int64)
        self.unranked = 0  # positives without a rank in the last evaluate()
        self.history: dict = {}
        self.unranked_history = np.zeros(0, dtype=np.int64)
        self._dev = self._fit = None

    # ------------------------------------------------------------------ layout of a result row
    @property
    def n_columns(self) -> int:
        return 3 * len(self.K) + 2

    def _split(self, table: np.ndarray) -> dict:
        """``{metric: [rows, width]}`` of result rows ``[rows, 3 n_K + 2]`` (DCG | Recall | MAP | MRR | AUC)."""
        n = len(self.K)
        at = {"DCG": (0, n), "Recall": (n, 2 * n), "MAP": (2 * n, 3 * n), "MRR": (3 * n, 3 * n + 1),
              "AUC": (3 * n + 1, 3 * n + 2)}
        return {m: table[:, at[m][0]:at[m][1]].copy() for m in self.used_metrics}

    # ------------------------------------------------------------------ device state
    def _bind(self, model):
        """The device-resident state for ``model`` (uploaded once, reused while the model's kind,
        runtime and shapes stay the same)."""
        torch = __import__("torch")
        is_fm = hasattr(model, "n_features")
        if is_fm and self.sides is None:
            raise ValueError("a FactorizationMachines needs sides=: its recommend.Sides")
        if not is_fm and self.sides is not None:
            raise ValueError("a LogisticMatrixFactorization takes no sides: give sides=None")
        n_users, n_items = rec.catalogue_shape(model, self.sides)
        if n_items != self.n_items:
            raise ValueError(f"the model ranks {n_items} items, the evaluator was given n_items={self.n_items}")
        if self.users.size and self.users.max() >= n_users:
            raise ValueError(f"a user id lies outside 0..{n_users - 1}")
        if self._excl is not None and self._excl[0].shape[0] != n_users + 1:
            raise ValueError(f"exclude lists {self._excl[0].shape[0] - 1} users, the model has {n_users}")
        rt = model._rt
        key = (id(rt), is_fm, n_users, int(model.n_factors))
        d = self._dev
        if d is None or d["key"] != key:
            n_sel, n_tgt = int(self._sel.shape[0]), int(self.items.shape[0])
            ws_m = C.c_int64(0)
            _lib.check(rt.lib.rfm_rank_metrics_workspace(n_sel, n_tgt, len(self.K), C.byref(ws_m)))
            d = {"key": key, "rt": rt, "n_sel": n_sel, "n_tgt": n_tgt, "ops": None,  # (the operands: the first _enqueue)
                 "sel": rt.upload(self._sel if n_sel else np.zeros(1, np.int32)), "indptr": rt.upload(self._indptr),
                 "items": rt.upload(self.items.astype(np.int32) if n_tgt else np.zeros(1, np.int32)),
                 "weights": None if self.pscores is None else rt.upload(1.0 / self.pscores if n_tgt else np.ones(1)),
                 "excl": rec._exclusions(rt, self._excl),
                 "ranks": rt.empty((max(n_tgt, 1),), torch.int32), "scores": rt.empty((max(n_tgt, 1),), torch.float64),
                 "cand": rt.empty((max(n_sel, 1),), torch.int32),
                 "ws_ranks": rt.empty((rec.ranks_workspace_bytes(n_sel, n_items, n_tgt),), torch.uint8),
                 "ws_metrics": rt.empty((int(ws_m.value),), torch.uint8),
                 "out": rt.empty((self.n_columns,), torch.float64), "counts": rt.empty((3,), torch.int64)}
            self._dev = d
        return d

    def _enqueue(self, model, d, weighted: bool, out_ptr: int, counts_ptr: int) -> None:
        """One evaluation of the model's current parameters, enqueued: the operands refreshed in
        place (FM: side sums), the two rank passes, the metrics; the result row goes to ``out_ptr``,
        the three counts to ``counts_ptr``."""
        rt = d["rt"]
        d["ops"] = rec.operands(model, self.sides, into=d["ops"])
        rec.enqueue_ranks(d["ops"], d["sel"], d["n_sel"], d["excl"], d["indptr"], d["items"], d["n_tgt"],
                          d["ws_ranks"], d["ranks"], d["scores"], d["cand"])
        _lib.check(rt.lib.rfm_rank_metrics(
            rt.ctx, d["indptr"].data_ptr(), d["n_sel"], d["n_tgt"], d["ranks"].data_ptr(), d["cand"].data_ptr(),
            d["weights"].data_ptr() if weighted and d["weights"] is not None else None, self._h_K.ctypes.data,
            len(self.K), d["ws_metrics"].data_ptr(), out_ptr, counts_ptr))

    # ------------------------------------------------------------------ one-shot
    def evaluate(self, model, estimator: str = "Naive") -> dict:
        """``{metric: [value per K]}`` (MRR, AUC: one value) of the model as it stands; only the
        result row comes back from the device.  Sets ``unranked``."""
        d = self._bind(model)
        self._enqueue(model, d, estimator == "IPS", d["out"].data_ptr(), d["counts"].data_ptr())
        d["rt"].sync()
        self.unranked = int(d["counts"].cpu().numpy()[2])
        return {m: v[0].tolist() for m, v in self._split(d["out"].cpu().numpy()[None, :]).items()}

    # ------------------------------------------------------------------ inside fit()
    def fit_begin(self, model, n_epochs: int) -> None:
        """Called by ``fit()`` before its first iteration: the device table of ``n_epochs`` result
        rows (NaN) and counts (-1)."""
        torch = __import__("torch")
        d = self._bind(model)
        rt = d["rt"]
        self._fit = {
            "model": model, "d": d, "n_epochs": int(n_epochs), "weighted": model.estimator == "IPS",
            "table": torch.full((int(n_epochs), self.n_columns), float("nan"), dtype=torch.float64, device=rt.torch_device),
            "counts": torch.full((int(n_epochs), 3), -1, dtype=torch.int64, device=rt.torch_device)}

    def fit_due(self, epoch: int) -> bool:
        return (epoch + 1) % self.every == 0 or epoch == self._fit["n_epochs"] - 1

    def fit_run_length(self, epoch: int) -> int:
        """Iterations from ``epoch`` up to and including the next one that is evaluated."""
        return min(self.every - epoch % self.every, self._fit["n_epochs"] - epoch)

    def fit_enqueue(self, epoch: int) -> None:
        """The evaluation after iteration ``epoch``, into that iteration's row of the device table."""
        f = self._fit
        self._enqueue(f["model"], f["d"], f["weighted"], f["table"].data_ptr() + epoch * self.n_columns * 8,
                      f["counts"].data_ptr() + epoch * 24)

    def fit_end(self) -> list:
        """Called by ``fit()`` after its synchronisation: the one download; fills ``history`` /
        ``unranked_history`` and returns the monitored column, one float per iteration."""
        f, self._fit = self._fit, None
        table, counts = f["table"].cpu().numpy(), f["counts"].cpu().numpy()
        self.history = self._split(table)
        self.unranked_history = counts[:, 2].astype(np.int64)
        done = np.flatnonzero(self.unranked_history >= 0)
        if done.size:
            self.unranked = int(self.unranked_history[done[-1]])
        metric, col = self._monitor
        return [float(v) for v in self.history[metric][:, col]]
