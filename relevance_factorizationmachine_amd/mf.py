"""``LogisticMatrixFactorization`` with the reference's surface
(``src/mf.py:16-170``) on top of the HIP kernels of librfm_hip.so.

The reference updates a batch strictly example by example
(``src/mf.py:97-108``).  That order is kept exactly: the host derives, per
batch, the level schedule (``rfm_mf_schedule``) under which every example runs
after the latest earlier example sharing its user or item, and the device
executes the levels in order (``csrc/rfm_mf.hip``).  ``fit_many`` runs several models that
share a training log and batch size on one such schedule at once, one chain each.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import numpy as np

from . import _lib, fold
from .base import LOSS_EPS, PointwiseBaseRecommender
from .evaluate import EvalLoop, FitHook, device_frame
from .optimizer import DeviceSGD, take_optimizer
from .runtime import BatchIdStream, Runtime, mf_cache_capacity, mf_schedule_ex, mf_schedule_rows


class _SchedulePipe:
    """Host side of the exact MF batches, off the critical path: a producer thread derives the
    level schedule of the coming iterations (``rfm_mf_schedule_ex``; ctypes releases the GIL)
    and packs it -- records, level pointers, cached items -- into a ring of PINNED host
    buffers; the consumer enqueues one asynchronous copy per iteration into the matching
    device slot and launches.  A host slot is handed back to the producer only after the copy
    out of it has completed (an event), a device slot is reused ``DEPTH`` iterations later on
    the same stream, i.e. after the kernels that read it.  ``with_rows``: the slot also carries
    the training-log row of every record (``rfm_mf_schedule_rows``, a schedule several models
    share)."""

    DEPTH = 8

    def __init__(self, rt: Runtime, batch_size: int, cache_cap: int, with_rows: bool = False):
        import queue

        import torch

        self.rt, self.B, self.cache_cap = rt, batch_size, cache_cap
        self.ex_bytes = 24 * batch_size
        self.lptr_off = (self.ex_bytes + 15) // 16 * 16
        self.cache_off = (self.lptr_off + 4 * (batch_size + 1) + 15) // 16 * 16
        self.rows_off = (self.cache_off + 4 * max(cache_cap, 1) + 15) // 16 * 16
        self.total = self.rows_off + (4 * batch_size if with_rows else 0)
        self.with_rows = with_rows
        self.host = [torch.empty(self.total, dtype=torch.uint8, pin_memory=True) for _ in range(self.DEPTH)]
        self.dev = [rt.empty((self.total,), torch.uint8) for _ in range(self.DEPTH)]
        self.free: "queue.Queue" = queue.Queue()
        for s in range(self.DEPTH):
            self.free.put((s, None))
        self.ready: "queue.Queue" = queue.Queue(maxsize=self.DEPTH)
        self.torch = torch

    def produce(self, epochs, schedule_fn) -> None:
        """Runs in the producer thread: ``schedule_fn(rows) -> (ex, level_ptr, cache_items)`` (with
        rows: ``(ex, ex_rows, level_ptr, cache_items)``) for every ``(epoch, rows, ids_ptr)`` of
        ``epochs``."""
        try:
            for epoch, rows, ids_ptr in epochs:
                slot, ev = self.free.get()
                if slot is None:
                    return
                if ev is not None:
                    ev.synchronize()  # the copy out of this host slot has completed
                ex, *ex_rows, level_ptr, cache_items = schedule_fn(rows)
                h = self.host[slot].numpy()
                if self.with_rows:
                    h[self.rows_off: self.rows_off + 4 * len(ex_rows[0])] = ex_rows[0].view(np.uint8)
                h[: self.ex_bytes] = ex.view(np.uint8)
                h[self.lptr_off: self.lptr_off + 4 * len(level_ptr)] = level_ptr.view(np.uint8)
                h[self.cache_off: self.cache_off + 4 * len(cache_items)] = cache_items.view(np.uint8)
                self.ready.put((epoch, ids_ptr, slot, len(level_ptr) - 1, len(cache_items)))
            self.ready.put(None)
        except BaseException as exc:  # noqa: BLE001 -- handed to the consumer
            self.ready.put(exc)
        finally:
            # the generator runs id_stream.chunks() in THIS thread: closing it here runs that
            # generator's cleanup (sampler thread stopped, pinned buffers released)
            close = getattr(epochs, "close", None)
            if close is not None:
                close()

    def take(self):
        """Next iteration: enqueues the copy and returns ``(epoch, ids_ptr, device ex ptr, HOST
        level_ptr ptr, device level_ptr ptr, n_levels, device cache ptr, n_cached, device ex_rows
        ptr, done)``; call ``done()`` after the launches that read the slot have been enqueued."""
        item = self.ready.get()
        if item is None:
            return None
        if isinstance(item, BaseException):
            raise item
        epoch, ids_ptr, slot, n_levels, n_cached = item
        self.dev[slot].copy_(self.host[slot], non_blocking=True)
        ev = self.torch.cuda.Event()
        ev.record()
        base, hbase = self.dev[slot].data_ptr(), self.host[slot].data_ptr()

        def done() -> None:
            self.free.put((slot, ev))

        return (epoch, ids_ptr, base, hbase + self.lptr_off, base + self.lptr_off, n_levels,
                base + self.cache_off, n_cached, base + self.rows_off, done)

    def stop(self) -> None:
        self.free.put((None, None))

    def run(self, epochs, schedule_fn, step) -> None:
        """The exact-mode loop of ``fit()`` and ``fit_many()``: the level schedules of the coming
        batches are derived and staged by a host thread while the GPU runs the batch before (the
        GPU never waits for them); ``step(*take())`` enqueues one iteration."""
        import threading

        worker = threading.Thread(target=self.produce, args=(epochs, schedule_fn), name="rfm-mf-schedule",
                                  daemon=True)
        worker.start()
        try:
            while True:
                got = self.take()
                if got is None:
                    break
                step(*got)
        finally:
            self.stop()
            self.rt.sync()
            worker.join(timeout=5.0)


class DevicePairs:
    """(user, item) pairs of a log in HBM as two int32 arrays."""

    def __init__(self, rt: Runtime, pairs: np.ndarray):
        pairs = np.asarray(pairs)
        if pairs.ndim != 2 or pairs.shape[1] < 2:
            raise ValueError("MF features must be an (N, 2) array of [user, item]")
        self.n = int(pairs.shape[0])
        self.h_users = np.ascontiguousarray(pairs[:, 0], dtype=np.int32)
        self.h_items = np.ascontiguousarray(pairs[:, 1], dtype=np.int32)
        self.users = rt.upload(self.h_users if self.n else np.zeros(1, np.int32))
        self.items = rt.upload(self.h_items if self.n else np.zeros(1, np.int32))


@dataclass
class FoldedRows:
    """New rows of one side of a trained MF model (``fold_in_users`` / ``fold_in_items``): device
    tensors ``rows [n_new, k]`` and ``bias [n_new]``, ``side`` "user" or "item"."""

    side: str
    rows: object
    bias: object
    rt: Runtime

    def __len__(self) -> int:
        return int(self.rows.shape[0])

    def numpy(self):
        """``(rows, bias)`` on the host, after the work enqueued so far."""
        self.rt.sync()
        return self.rows.cpu().numpy(), self.bias.cpu().numpy()


@dataclass
class LogisticMatrixFactorization(PointwiseBaseRecommender):
    """Logistic matrix factorisation trained by per-example SGD on an MI355X.

    Args (``src/mf.py:20-32``): n_users, n_items, reg (L2 on touched rows),
    alpha (init scale), evaluator (optional ``ValEvaluator``-like object).
    """

    n_users: int
    n_items: int
    reg: float
    alpha: float = 4.0
    evaluator: Optional[object] = None

    # Not a constructor argument.  False (default): the reference's strictly
    # sequential per-example updates, reproduced exactly through the level
    # schedule.  True: HOGWILD-style unordered updates (rfm_mf_sgd_hogwild) -- a
    # throughput mode whose parameters do NOT match the reference to 1e-5.
    hogwild = False
    # Not a constructor argument: a ValEvaluator-like ``evaluator`` (see evaluate.py) is
    # computed on the device; False keeps the host callback for every evaluator.
    device_evaluator = True
    # Not constructor arguments: the update rule of fit() -- "sgd" (the reference's, theta -= lr * g)
    # or "adagrad" (G += g * g; theta -= lr * g / (sqrt(G) + adagrad_eps) for each of an example's four
    # updates in the reference's order, accumulators G of the parameters' shapes that start at
    # adagrad_init and persist across fit() calls: DESIGN §8 N20).  Exact mode only; fit_many, the
    # user-partitioned fit and fold-in take the SGD step only.
    optimizer = "sgd"
    adagrad_eps = 1e-10
    adagrad_init = 0.0

    def __post_init__(self) -> None:
        # src/mf.py:34-66 -- the reference's NumPy calls, in its draw order
        np.random.seed(self.seed)
        limit = self.alpha * np.sqrt(6 / self.n_factors)
        P = np.random.uniform(low=-limit, high=limit, size=(self.n_users, self.n_factors))
        Q = np.random.uniform(low=-limit, high=limit, size=(self.n_items, self.n_factors))
        b_u = np.random.normal(scale=0.001, size=self.n_users)
        b_i = np.random.normal(scale=0.001, size=self.n_items)

        self._rt = Runtime.get()
        self.P = DeviceSGD(self._rt, P, self.lr)
        self.Q = DeviceSGD(self._rt, Q, self.lr)
        self.b_u = DeviceSGD(self._rt, b_u, self.lr)
        self.b_i = DeviceSGD(self._rt, b_i, self.lr)

        if self.evaluator is not None:
            self.val_metrics = []
            self.model_name = "MF"

    def _check_ids(self, pairs: DevicePairs) -> None:
        if pairs.n == 0:
            return
        if pairs.h_users.min() < 0 or pairs.h_users.max() >= self.n_users:
            raise IndexError("user id out of range")
        if pairs.h_items.min() < 0 or pairs.h_items.max() >= self.n_items:
            raise IndexError("item id out of range")

    # ------------------------------------------------------------------ fit
    def fit(self, train: dict, val: dict) -> tuple:
        """src/mf.py:68-134."""
        rt = self._rt
        take_optimizer(self, ("P", "Q", "b_u", "b_i"), inexact=self.hogwild)
        # global bias: mean of the training labels (src/mf.py:84)
        self.b = np.mean(train["labels"])
        n_rows = int(np.asarray(train["features"]).shape[0])
        if self.n_epochs <= 0:
            return [], []
        # resample(..., random_state=epoch) ids (src/mf.py:88-95), sampled chunk by chunk on
        # the host while the GPU works on the chunk before
        id_stream = BatchIdStream(rt, n_rows, self.batch_size, self.n_epochs)
        try:
            return self._fit(train, val, id_stream)
        finally:
            id_stream.close()  # (its sampler thread runs from the constructor on)

    def _fit(self, train: dict, val: dict, id_stream: BatchIdStream) -> tuple:
        rt = self._rt
        self._keep_ids = []

        tr = DevicePairs(rt, train["features"])
        va = DevicePairs(rt, val["features"])
        self._check_ids(tr)
        self._check_ids(va)
        y = rt.upload(np.asarray(train["labels"]), dtype=np.float64)
        p = rt.upload(np.asarray(train["pscores"]), dtype=np.float64)
        vy = rt.upload(np.asarray(val["labels"]), dtype=np.float64)
        vp = rt.upload(np.asarray(val["pscores"]), dtype=np.float64)
        tl = rt.empty((self.n_epochs,), y.dtype)
        vl = rt.empty((self.n_epochs,), y.dtype)
        if va.n == 0:  # the reference's mean over no rows is nan (src/base.py:61)
            vl.fill_(float("nan"))
        params = (self.P.dev.data_ptr(), self.Q.dev.data_ptr(), self.b_u.dev.data_ptr(),
                  self.b_i.dev.data_ptr())
        b = float(self.b)
        adagrad = take_optimizer(self, ("P", "Q", "b_u", "b_i"), inexact=self.hogwild)
        h_y = np.ascontiguousarray(train["labels"], dtype=np.float64)
        h_p = np.ascontiguousarray(train["pscores"], dtype=np.float64)
        # item rows the sequential kernel may keep in LDS (rows + bias, 32 KiB)
        cache_cap = mf_cache_capacity(self.n_factors)

        def make_loop(evaluator):
            # ValEvaluator's IPS-DCG@k from scores that stay in HBM (rfm_val_dcg)
            ev_X = evaluator.features[self.model_name]
            frame = device_frame(rt, evaluator, self.estimator, int(np.asarray(ev_X).shape[0]))
            if frame is None:
                return None
            ev_pairs = DevicePairs(rt, ev_X)
            self._check_ids(ev_pairs)
            return EvalLoop(rt, frame, evaluator, self.estimator, self.n_epochs, log=ev_pairs)

        hook = FitHook(self, self.n_epochs, self.predict, make_loop)

        def after_sgd(epoch: int, ids_ptr: int) -> None:
            # train loss on the same batch with the updated parameters (src/mf.py:110-116)
            _lib.check(rt.lib.rfm_mf_predict_loss(
                rt.ctx, tr.users.data_ptr(), tr.items.data_ptr(), y.data_ptr(), p.data_ptr(),
                ids_ptr, self.batch_size, *params, b, self.n_factors, LOSS_EPS, None,
                tl.data_ptr() + epoch * 8))
            if va.n > 0:
                _lib.check(rt.lib.rfm_mf_predict_loss(
                    rt.ctx, va.users.data_ptr(), va.items.data_ptr(), vy.data_ptr(), vp.data_ptr(),
                    None, va.n, *params, b, self.n_factors, LOSS_EPS, None, vl.data_ptr() + epoch * 8))
            if hook.loop is not None:
                ev_pairs = hook.loop.log
                _lib.check(rt.lib.rfm_mf_predict(
                    rt.ctx, ev_pairs.users.data_ptr(), ev_pairs.items.data_ptr(), None, ev_pairs.n,
                    *params, b, self.n_factors, hook.loop.slot(epoch).data_ptr()))
                hook.loop.measure(epoch)
            hook.ran(epoch, 1)

        if self.hogwild:
            for epoch, rows, ids_ptr in self._epochs(id_stream):
                _lib.check(rt.lib.rfm_mf_sgd_hogwild(
                    rt.ctx, tr.users.data_ptr(), tr.items.data_ptr(), y.data_ptr(), p.data_ptr(),
                    ids_ptr, self.batch_size, *params, b, self.n_factors, float(self.lr),
                    float(self.reg)))
                after_sgd(epoch, ids_ptr)
        else:
            # exact mode (_SchedulePipe.run)
            pipe = _SchedulePipe(rt, self.batch_size, cache_cap)

            def schedule(rows):
                return mf_schedule_ex(tr.h_users[rows], tr.h_items[rows], h_y[rows], h_p[rows],
                                      self.n_users, self.n_items, cache_cap)

            # the SGD fit runs rfm_mf_sgd_levels_ex; the other rule is the same schedule through
            # rfm_mf_sgd_levels_opt, whose arguments end with kind, accumulators and eps
            levels, rule = rt.lib.rfm_mf_sgd_levels_ex, ()
            if adagrad:
                levels = rt.lib.rfm_mf_sgd_levels_opt
                rule = (_lib.OPT_ADAGRAD, *(h.acc.data_ptr() for h in (self.P, self.Q, self.b_u, self.b_i)),
                        float(self.adagrad_eps))

            def step(epoch, ids_ptr, d_ex, h_lptr, d_lptr, n_levels, d_cache, n_cached, _d_rows, done):
                _lib.check(levels(rt.ctx, d_ex, h_lptr, d_lptr, n_levels, d_cache, n_cached, *params, b,
                                  self.n_factors, float(self.lr), float(self.reg), *rule))
                done()
                after_sgd(epoch, ids_ptr)

            pipe.run(self._epochs(id_stream), schedule, step)
        rt.sync()
        self._keep_ids = []
        hook.finish()
        return tl.cpu().numpy().tolist(), vl.cpu().numpy().tolist()

    def _epochs(self, id_stream: BatchIdStream):
        """``(epoch, host row ids, device address of the ids)`` of every iteration."""
        for first, host_ids, dev_ids in id_stream.chunks():
            self._keep_ids.append(dev_ids)  # launches enqueued later still read these ids
            for j in range(host_ids.shape[0]):
                yield first + j, host_ids[j], dev_ids.data_ptr() + j * self.batch_size * 4

    # -------------------------------------------------------------- predict
    def predict(self, X) -> np.ndarray:
        """src/mf.py:136-152 -- scores of (user, item) pairs."""
        rt = self._rt
        if not hasattr(self, "b"):
            # the reference's global bias exists only after fit() (src/mf.py:84)
            raise AttributeError("'LogisticMatrixFactorization' object has no attribute 'b'")
        pairs = DevicePairs(rt, X)
        self._check_ids(pairs)
        out = rt.empty((pairs.n,), self.P.dev.dtype)
        _lib.check(rt.lib.rfm_mf_predict(
            rt.ctx, pairs.users.data_ptr(), pairs.items.data_ptr(), None, pairs.n,
            self.P.dev.data_ptr(), self.Q.dev.data_ptr(), self.b_u.dev.data_ptr(),
            self.b_i.dev.data_ptr(), float(self.b), self.n_factors, out.data_ptr()))
        rt.sync()
        return out.cpu().numpy()

    # -------------------------------------------------------------- fold-in
    def _fold_in(self, side: int, data: dict, n_new: int, n_passes: int, init, group=None, check=True) -> FoldedRows:
        """New rows of ``side`` (0: users, 1: items) trained against the fixed other side
        (``rfm_mf_fold_in``): enqueued on the runtime's stream, no host wait."""
        import torch

        rt = self._rt
        if not hasattr(self, "b"):
            # the reference's global bias exists only after fit() (src/mf.py:84)
            raise AttributeError("'LogisticMatrixFactorization' object has no attribute 'b'")
        F, fb, n_fixed = ((self.Q, self.b_i, self.n_items), (self.P, self.b_u, self.n_users))[side]
        examples = fold.grouped_examples(rt, data, n_new, n_fixed, side, n_passes, group, check)
        n_new, kf = int(n_new), int(self.n_factors)
        start = fold.initial_state(init, n_new, kf, ("rows", "bias"))
        if start is None:
            rows = torch.zeros((n_new, kf), dtype=torch.float64, device=rt.torch_device)
            bias = torch.zeros((n_new,), dtype=torch.float64, device=rt.torch_device)
        else:
            rows, bias = rt.upload(start[0]), rt.upload(start[1])
        if n_new and int(n_passes):
            dev = examples()
            _lib.check(rt.lib.rfm_mf_fold_in(
                rt.ctx, *(d.data_ptr() for d in dev), n_new, F.dev.data_ptr(), fb.dev.data_ptr(), n_fixed,
                float(self.b), kf, float(self.lr), float(self.reg), int(n_passes), rows.data_ptr(),
                bias.data_ptr()))
        return FoldedRows(("user", "item")[side], rows, bias, rt)

    def fold_in_users(self, data: dict, n_new: int, n_passes: int, init=None, group=None, check=True) -> FoldedRows:
        """Rows and biases for ``n_new`` users who arrived after the fit, by the reference's own
        per-example update (``src/mf.py:99-108``) with ``Q, b_i`` held fixed.  ``data`` as ``fit()``
        takes it: the user column of ``features`` holds new-user indices 0..n_new-1, the item column
        known item ids; a user's examples are taken in input order, ``n_passes`` times.  ``init``:
        ``(rows [n_new, k], bias [n_new])`` to start from (default zeros).  The model is not
        written; serve the result through ``new_users=`` or ``append_users`` it.  That is the SGD
        step whatever ``optimizer`` the model was fitted with: a new row has no history of gradients,
        and ``append_users`` starts its accumulators at ``adagrad_init``.
        ``group``: where the examples are grouped by user -- "host" (NumPy, then
        uploaded), "device" (``rfm_fold_group``; the pieces of ``data`` may be tensors on the device,
        host pieces are uploaded as they are), None: "device" if ``data["features"]`` is a device
        tensor, else "host"; the result has the same bits either way.  ``check`` (device grouping
        only): True waits once for the device's id check and raises the host path's ``IndexError``;
        False waits for nothing, and an example with an id out of range is left out."""
        return self._fold_in(0, data, n_new, n_passes, init, group, check)

    def fold_in_items(self, data: dict, n_new: int, n_passes: int, init=None, group=None, check=True) -> FoldedRows:
        """``fold_in_users`` with the sides exchanged: the item column of ``features`` holds new-item
        indices, the user column known user ids, and ``P, b_u`` are held fixed."""
        return self._fold_in(1, data, n_new, n_passes, init, group, check)

    def _append(self, folded: FoldedRows, side: str, M: DeviceSGD, bias: DeviceSGD) -> np.ndarray:
        if not isinstance(folded, FoldedRows) or folded.side != side:
            raise TypeError(f"append_{side}s takes the FoldedRows of fold_in_{side}s")
        if tuple(folded.rows.shape[1:]) != (self.n_factors,):
            raise ValueError(f"folded rows of {tuple(folded.rows.shape)} for a model of {self.n_factors} factors")
        first = int(M.dev.shape[0])
        M.append(folded.rows)
        bias.append(folded.bias)
        return np.arange(first, first + len(folded))

    def append_users(self, folded: FoldedRows) -> np.ndarray:
        """Grows ``P, b_u`` and ``n_users`` by folded user rows (and, under ``optimizer = "adagrad"``,
        their accumulators by ``adagrad_init``); returns their user ids."""
        ids = self._append(folded, "user", self.P, self.b_u)
        self.n_users += len(folded)
        return ids

    def append_items(self, folded: FoldedRows) -> np.ndarray:
        """Grows ``Q, b_i`` and ``n_items`` by folded item rows (and, under ``optimizer = "adagrad"``,
        their accumulators by ``adagrad_init``); returns their item ids."""
        ids = self._append(folded, "item", self.Q, self.b_i)
        self.n_items += len(folded)
        return ids

    # ------------------------------------------------------------ catalogue
    # new_users: the FoldedRows of fold_in_users stand in for P, b_u -- ``users`` and ``exclude``
    # then index the folded rows, and the model is not touched
    def score_pairs(self, users=None, new_users=None) -> np.ndarray:
        """``predict()`` of every (user, item) pair as a ``[n_users (or len(users)), n_items]``
        matrix: one dense product (recommend.py; src/mf.py:136-170 restated)."""
        from . import recommend as rec

        return rec.score_pairs(*rec.operands(self, new_users=new_users), users)

    def recommend(self, k: int, users=None, exclude=None, new_users=None):
        """The ``k`` (1..64) best items per user: ``(items int32 [n, k], scores float64 [n, k])``,
        ranked by logit (ties: higher item index first); ``exclude``: CSR by user id."""
        from . import recommend as rec

        return rec.topk(*rec.operands(self, new_users=new_users), k, users, exclude)

    def rank_items(self, users, items, exclude=None, new_users=None):
        """Where the pairs ``(users[n], items[n])`` land in their users' ranking of all items:
        ``(ranks int32 [n], scores float64 [n], candidates int32 [n])`` in input order, ranks
        0-based under ``recommend()``'s order, at any depth (recommend.py)."""
        from . import recommend as rec

        return rec.rank_items(*rec.operands(self, new_users=new_users), users, items, exclude)

    def rank_catalogue(self, depth: int, users=None, exclude=None, new_users=None):
        """Every user's ranking of all items down to ``depth`` (any integer >= 1): ``(items int32
        [n, depth], scores float64 [n, depth], n_ranked int32 [n])`` under ``recommend()``'s
        order, short rows padded with item -1 / score NaN (recommend.py)."""
        from . import recommend as rec

        return rec.rank_catalogue(*rec.operands(self, new_users=new_users), depth, users, exclude)

    def recommend_diverse(self, k: int, depth=None, trade_off=0.5, users=None, exclude=None, metric="cosine",
                          item_penalty=None, new_users=None):
        """``k`` (1..64) of each user's ``depth`` best items (default ``min(n_items, max(64, 4 k))``, at
        most 1 024), chosen greedily by Maximal Marginal Relevance: ``(items int32 [n, k], scores
        float64 [n, k], values float64 [n, k])`` in the order chosen.  A pick maximises ``trade_off *
        score - item_penalty[item] - (1 - trade_off) * max similarity to the picks before it``, the
        similarity the cosine (``metric="dot"``: the dot product) of rows of ``Q``; ``trade_off=1``
        without a penalty is ``recommend(k)``.  Short rows pad with item -1 / NaN (recommend.diverse)."""
        from . import recommend as rec

        return rec.diverse(self, None, k, depth, trade_off, users, exclude, metric, item_penalty, new_users)

    # the item -> users direction.  new_items: the FoldedRows of fold_in_items stand
    # in for Q, b_i -- ``items`` and the item axis of ``exclude`` then index the folded rows; new_users
    # as above; the model is not touched.  ``exclude`` is the matrix recommend() takes, by user id
    def recommend_users(self, k: int, items=None, exclude=None, new_items=None, new_users=None):
        """The ``k`` (1..64) best users per item: ``(users int32 [n, k], scores float64 [n, k])``,
        ranked by logit (ties: higher user index first), scores ``sigmoid(logit)`` as ``predict()``
        gives them -- the score of (item i, user u) has the bytes ``recommend()`` gives (u, i);
        short lists are padded with user -1 / score NaN."""
        from . import recommend as rec

        return rec.topk_users(*rec.operands(self, new_users=new_users, new_items=new_items), k, items, exclude)

    def rank_users(self, items, users, exclude=None, new_items=None, new_users=None):
        """Where user ``users[n]`` stands among all users in item ``items[n]``'s ranking:
        ``(ranks int32 [n], scores float64 [n], candidates int32 [n])`` in input order, ranks
        0-based under ``recommend_users()``'s order, at any depth (recommend.py)."""
        from . import recommend as rec

        return rec.rank_users(*rec.operands(self, new_users=new_users, new_items=new_items), items, users, exclude)

    def rank_audience(self, depth: int, items=None, exclude=None, new_items=None, new_users=None,
                      workspace_bytes=None):
        """Every item's ranking of all users down to ``depth`` (any integer >= 1): ``(users int32
        [n, depth], scores float64 [n, depth], n_ranked int32 [n])`` under ``recommend_users()``'s
        order, short rows padded with user -1 / score NaN (recommend.py)."""
        from . import recommend as rec

        return rec.rank_audience(*rec.operands(self, new_users=new_users, new_items=new_items), depth, items, exclude,
                                 workspace_bytes)

    # new_items / new_users: the FoldedRows of the matching fold_in_* are the queries against the
    # model's own rows -- ``items`` / ``users`` then index the folded rows, which have no self
    def similar_items(self, k: int, items=None, metric="cosine", exclude=None, include_self=False, new_items=None):
        """The ``k`` (1..64) items most like each item: ``(items int32 [n, k], values float64 [n, k])``,
        the cosine (``metric="dot"``: the dot product) of rows of ``Q``, best first, ties: higher
        index first, an item never its own neighbour unless ``include_self``; ``exclude``: CSR by
        item id.  Similarity is in factor space only: ``b_i`` plays no part (recommend.neighbours)."""
        from . import recommend as rec

        return rec.similar(self, "item", k, items, metric, exclude, include_self, new_items)

    def similar_users(self, k: int, users=None, metric="cosine", exclude=None, include_self=False, new_users=None):
        """``similar_items`` for the rows of ``P``: the ``k`` users most like each user, in factor
        space only (``b_u`` plays no part)."""
        from . import recommend as rec

        return rec.similar(self, "user", k, users, metric, exclude, include_self, new_users)


# ---------------------------------------------------------------------------
# several models on one training log
# ---------------------------------------------------------------------------
_SHARED_FIELDS = ("n_users", "n_items", "n_factors", "batch_size", "n_epochs")


def _one_per_model(split, n: int, name: str) -> list:
    if isinstance(split, dict):
        return [split] * n
    split = list(split)
    if len(split) != n:
        raise ValueError(f"fit_many: {name} must be one dict or one per model ({len(split)} for {n} models)")
    return split


def _same_features(splits: list, name: str) -> None:
    first = np.asarray(splits[0]["features"])
    for s in splits[1:]:
        if s is not splits[0] and not np.array_equal(first, np.asarray(s["features"])):
            raise ValueError(f"fit_many: the models' {name} features differ (one schedule serves one log)")


def _device_table(rt: Runtime, structs):
    """A ctypes array of structs (or of pointers) as bytes on the device."""
    return rt.upload(np.frombuffer(bytes(structs), dtype=np.uint8).copy())


def fit_many(models, train, val) -> list:
    """``model.fit(train, val)`` of every model of ``models`` at once, one chain each:
    ``[(train_loss, val_loss), ...]`` in model order, and every model left exactly as its own
    ``fit()`` leaves it (``b``, ``P``, ``Q``, ``b_u``, ``b_i``, ``val_metrics`` and the evaluator
    counters), bit for bit.

    ``train`` / ``val``: one dict shared by all, or a list with one per model.  The models must
    agree in ``n_users``, ``n_items``, ``n_factors``, ``batch_size``, ``n_epochs`` and in the
    ``features`` of both splits (and of their evaluators): they then draw the same batch ids in
    every iteration (``resample(..., random_state=epoch)``, ``src/mf.py:88-95``) and share the level
    schedule, which is derived and uploaded once per iteration (``rfm_mf_schedule_rows``,
    ``rfm_mf_sgd_levels_many``).  They may differ in ``seed``, ``alpha``, ``lr``, ``reg``,
    ``estimator``, labels, propensities and evaluator instance.  Exact mode and the SGD rule only; an evaluator must
    be one the device computes (``evaluate.recognise``) -- anything else is a ``ValueError``."""
    from .evaluate import CatalogueValEvaluator, recognise

    models = list(models)
    n = len(models)
    if n == 0:
        return []
    if n > _lib.MF_MAX_MODELS:
        raise ValueError(f"fit_many: {n} models, at most {_lib.MF_MAX_MODELS} in one call")
    if any(not isinstance(m, LogisticMatrixFactorization) for m in models):
        raise TypeError("fit_many takes LogisticMatrixFactorization models")
    if len({id(m) for m in models}) != n:
        raise ValueError("fit_many: a model is listed twice")
    trains, vals = _one_per_model(train, n, "train"), _one_per_model(val, n, "val")
    m0 = models[0]
    for name in _SHARED_FIELDS:
        if any(getattr(m, name) != getattr(m0, name) for m in models):
            raise ValueError(f"fit_many: the models differ in {name}")
    if any(m.hogwild for m in models):
        raise ValueError("fit_many: hogwild = True has no order to share; use fit()")
    if any(m.optimizer != "sgd" for m in models):
        # (rfm_mf_model is a fixed ABI struct without accumulators: DESIGN.md 8 N20)
        raise ValueError("fit_many applies the SGD rule only; fit() a model whose optimizer is 'adagrad'")
    _same_features(trains, "train")
    _same_features(vals, "val")
    with_ev = [m.evaluator is not None for m in models]
    if any(with_ev):
        if not all(with_ev):
            raise ValueError("fit_many: evaluator on some models only; give every model one or use fit()")
        ev_X = np.asarray(m0.evaluator.features[m0.model_name])
        for m in models:
            ev = m.evaluator
            if isinstance(ev, CatalogueValEvaluator):
                raise ValueError("fit_many: a CatalogueValEvaluator evaluator is not served; use fit()")
            if not m.device_evaluator:
                raise ValueError("fit_many: device_evaluator = False (a host callback per iteration); use fit()")
            got = recognise(ev, m.estimator)
            X = np.asarray(ev.features[m.model_name])
            if got is None or got[0].shape[0] != X.shape[0]:
                raise ValueError("fit_many: an evaluator that is a host callback is not served; use fit()")
            if ev is not m0.evaluator and not np.array_equal(ev_X, X):
                raise ValueError("fit_many: the models' evaluator features differ")
    for m, t in zip(models, trains):
        m.b = np.mean(t["labels"])  # global bias: mean of the training labels (src/mf.py:84)
    if m0.n_epochs <= 0:
        return [([], []) for _ in models]
    n_rows = int(np.asarray(trains[0]["features"]).shape[0])
    id_stream = BatchIdStream(m0._rt, n_rows, m0.batch_size, m0.n_epochs)
    try:
        return _fit_many(models, trains, vals, id_stream)
    finally:
        id_stream.close()


def _fit_many(models: list, trains: list, vals: list, id_stream: BatchIdStream) -> list:
    import torch

    m0, n = models[0], len(models)
    rt, B, kf, n_epochs = m0._rt, m0.batch_size, m0.n_factors, m0.n_epochs
    m0._keep_ids = []
    tr = DevicePairs(rt, trains[0]["features"])
    va = DevicePairs(rt, vals[0]["features"])
    m0._check_ids(tr)
    m0._check_ids(va)

    # label and propensity vectors, each distinct pair uploaded once; label / propensity over the
    # training log divided once per distinct pair, on the host as rfm_mf_schedule_ex divides it
    keep, vectors, ratios = [], {}, {}

    def vector(a):
        if id(a) not in vectors:
            keep.append(a)
            vectors[id(a)] = rt.upload(np.asarray(a), dtype=np.float64)
        return vectors[id(a)]

    def ratio(y, p):
        key = (id(y), id(p))
        if key not in ratios:
            keep.extend((y, p))
            ratios[key] = rt.upload(np.ascontiguousarray(y, dtype=np.float64) / np.ascontiguousarray(p, dtype=np.float64))
        return ratios[key]

    model_rows, tr_labels, va_labels = [], [], []
    for m, t, v in zip(models, trains, vals):
        ry = ratio(t["labels"], t["pscores"])
        model_rows.append(_lib.MfModel(m.P.dev.data_ptr(), m.Q.dev.data_ptr(), m.b_u.dev.data_ptr(),
                                       m.b_i.dev.data_ptr(), ry.data_ptr(), float(m.b), float(m.lr), float(m.reg)))
        tr_labels.append(_lib.MfLabels(vector(t["labels"]).data_ptr(), vector(t["pscores"]).data_ptr()))
        va_labels.append(_lib.MfLabels(vector(v["labels"]).data_ptr(), vector(v["pscores"]).data_ptr()))
    # the device tables are built here, once: no launch of the fit rewrites them
    d_models = _device_table(rt, (_lib.MfModel * n)(*model_rows))
    d_tr_labels = _device_table(rt, (_lib.MfLabels * n)(*tr_labels))
    d_va_labels = _device_table(rt, (_lib.MfLabels * n)(*va_labels))
    tl = rt.empty((n, n_epochs), torch.float64)
    vl = rt.empty((n, n_epochs), torch.float64)
    if va.n == 0:  # the reference's mean over no rows is nan (src/base.py:61)
        vl.fill_(float("nan"))
    cache_cap = mf_cache_capacity(kf)

    def make_loop(m):
        def make(evaluator):
            ev_X = evaluator.features[m.model_name]
            frame = device_frame(rt, evaluator, m.estimator, int(np.asarray(ev_X).shape[0]))
            return EvalLoop(rt, frame, evaluator, m.estimator, n_epochs)
        return make

    hooks = [FitHook(m, n_epochs, m.predict, make_loop(m)) for m in models]
    loops = [h.loop for h in hooks if h.loop is not None]
    d_slots = ev_pairs = None
    if loops:
        if len(loops) != n or len({(lp.chunk, int(lp.scores.shape[1])) for lp in loops}) != 1:
            raise ValueError("fit_many: the models' evaluator frames differ in shape; use fit()")
        ev_pairs = DevicePairs(rt, m0.evaluator.features[m0.model_name])
        m0._check_ids(ev_pairs)
        d_slots = _device_table(rt, (_lib.C.c_void_p * n)(*(lp.scores.data_ptr() for lp in loops)))
        slot_stride = int(loops[0].scores.shape[1])

    def schedule(rows):
        return mf_schedule_rows(tr.h_users[rows], tr.h_items[rows], rows, m0.n_users, m0.n_items, cache_cap)

    lib, ctx = rt.lib, rt.ctx
    models_ptr = d_models.data_ptr()

    def step(epoch, ids_ptr, d_ex, h_lptr, d_lptr, n_levels, d_cache, n_cached, d_rows, done):
        _lib.check(lib.rfm_mf_sgd_levels_many(ctx, d_ex, d_rows, h_lptr, d_lptr, n_levels, d_cache, n_cached,
                                              models_ptr, n, kf))
        done()
        # train loss on the same batch with the updated parameters (src/mf.py:110-116)
        _lib.check(lib.rfm_mf_predict_loss_many(
            ctx, tr.users.data_ptr(), tr.items.data_ptr(), d_tr_labels.data_ptr(), ids_ptr, B, models_ptr, n, kf,
            LOSS_EPS, None, 0, tl.data_ptr() + epoch * 8, n_epochs))
        if va.n > 0:
            _lib.check(lib.rfm_mf_predict_loss_many(
                ctx, va.users.data_ptr(), va.items.data_ptr(), d_va_labels.data_ptr(), None, va.n, models_ptr, n,
                kf, LOSS_EPS, None, 0, vl.data_ptr() + epoch * 8, n_epochs))
        if loops:
            _lib.check(lib.rfm_mf_predict_many(
                ctx, ev_pairs.users.data_ptr(), ev_pairs.items.data_ptr(), None, ev_pairs.n, models_ptr, n, kf,
                d_slots.data_ptr(), (epoch % loops[0].chunk) * slot_stride))
            for lp in loops:
                lp.measure(epoch)
        for h in hooks:
            h.ran(epoch, 1)

    _SchedulePipe(rt, B, cache_cap, with_rows=True).run(m0._epochs(id_stream), schedule, step)
    rt.sync()
    m0._keep_ids = []
    for h in hooks:
        h.finish()
    tl, vl = tl.cpu().numpy(), vl.cpu().numpy()
    return [(tl[j].tolist(), vl[j].tolist()) for j in range(n)]
