"""Catalogue scoring and top-K recommendation: every (user, item) pair of a
trained model without the design matrix of the pairs.

The FM rows the reference's loaders build are "the user's entries + the item's entries" on
disjoint columns (``features.fm_features_kuairec`` / ``fm_features_coat``: every segment is keyed
by the user id or by the item id), ``x(u,i) = xu(u) + xi(i)``.  With
``a_u = sum_j xu_j V[j,:]``, ``b_i = sum_j xi_j V[j,:]`` and, per side,
``L(x) = w.x + 0.5 sum_f((sum_j x_j V[j,f])^2 - sum_j x_j^2 V[j,f]^2)`` the reference's logit
(``src/fm.py:124-132``) is exactly ``w0 + L(xu) + L(xi) + a_u . b_i``; MF's
(``src/mf.py:154-170``) has the same shape with ``a = P``, ``b = Q``, ``L = b_u``, ``b_i`` and the
constant ``b``.  :class:`Sides` holds the two side matrices in HBM; ``FactorizationMachines.
recommend`` / ``score_pairs`` and their MF counterparts call the functions below.

Ranking is by the LOGIT under the total order (logit descending, then item index descending) --
``np.argsort(logit, kind="stable")[::-1][:k]``; the probabilities saturate to exactly 0.0 / 1.0 and
would tie.  The returned scores are probabilities, ``sigmoid(logit)``, as ``predict()`` gives.
``rank_items`` is the opposite question under the same order: the position of
given (user, item) pairs in the user's ranking of the whole catalogue, at any depth.
``rank_catalogue`` is ``topk`` without the limit of 64: the items at positions
0 .. depth-1, up to the user's full ordering of the catalogue.
``neighbours`` asks the tables themselves: the rows of ``B`` (or of ``A``) nearest to
each other by cosine or dot product, under the same order, with the value itself returned.
``topk_users`` / ``rank_users`` / ``rank_audience`` are ``topk`` / ``rank_items`` /
``rank_catalogue`` for "this item, which users?": the same pair has the same logit, bit for bit, in
both directions, ties go to the higher USER index, and ``exclude`` stays the matrix by user id.
``diverse`` / ``diversify`` re-rank: ``k`` of each user's ``depth`` most relevant items,
chosen greedily by Maximal Marginal Relevance against the rows of the item table.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Tuple

import numpy as np

from . import _lib
from .runtime import DeviceCSR, Runtime

MAX_K = 64
# rank_catalogue(workspace_bytes=None): the most workspace it takes by itself.  One row of logits per
# user of a block, so 1 GiB is a single block up to 12 500 users x 10 728 items (the reference's
# KuaiRec catalogue: 7 176 users) and about 1 300 users a block at 100 000 items -- hundreds of
# workgroups per launch either way, on a device with 288 GB.  Never below the ABI's minimum.
ORDER_WORKSPACE_BYTES = 1 << 30


def pad4(n_factors: int) -> int:
    """Row stride of the dense operands: the factor count rounded up to a multiple of 4."""
    return (int(n_factors) + 3) // 4 * 4


def topk_workspace_bytes(n_sel_users: int, n_items: int, k: int) -> int:
    """Bytes of workspace ``rfm_pair_topk`` needs (host only); ``ValueError`` unless 1 <= k <= 64."""
    out = C.c_int64(0)
    _lib.check(_lib.load().rfm_pair_topk_workspace(int(n_sel_users), int(n_items), int(k), C.byref(out)))
    return int(out.value)


def _stored_columns(X) -> np.ndarray:
    if isinstance(X, DeviceCSR):
        idx = X.h_indices if X.h_indices is not None else X.indices.cpu().numpy()[: X.nnz]
    else:
        idx = X.indices
    return np.unique(np.asarray(idx))


class Sides:
    """The user side and the item side of a design matrix whose pair rows are
    ``user_rows[u] + item_rows[i]``: two CSR matrices (scipy or ``DeviceCSR``), both ``n_features``
    wide, with DISJOINT column support -- a column stored on both sides makes the identity false
    and is a ``ValueError``.  Uploaded once (on first use), reusable across models and calls."""

    def __init__(self, user_rows, item_rows):
        if len(user_rows.shape) != 2 or len(item_rows.shape) != 2 or user_rows.shape[1] != item_rows.shape[1]:
            raise ValueError(f"the two sides must be matrices of the same width, got {tuple(user_rows.shape)} "
                             f"and {tuple(item_rows.shape)}")
        if not isinstance(user_rows, DeviceCSR):
            user_rows = user_rows.tocsr()
        if not isinstance(item_rows, DeviceCSR):
            item_rows = item_rows.tocsr()
        both = np.intersect1d(_stored_columns(user_rows), _stored_columns(item_rows))
        if both.size:
            raise ValueError(f"column {int(both[0])} is stored on the user side and on the item side "
                             f"({both.size} such columns): pair rows are not user_rows[u] + item_rows[i]")
        self.n_users, self.n_items = int(user_rows.shape[0]), int(item_rows.shape[0])
        self.n_features = int(user_rows.shape[1])
        if self.n_users < 1 or self.n_items < 1:
            raise ValueError("a side without rows")
        self._host = (user_rows, item_rows)
        self._dev = None

    def device(self, rt: Runtime) -> Tuple[DeviceCSR, DeviceCSR]:
        if self._dev is None:
            self._dev = tuple(X if isinstance(X, DeviceCSR) else DeviceCSR(rt, X) for X in self._host)
        return self._dev


class Operands(NamedTuple):
    """The dense problem ``logit(u,i) = c + LU[u] + LI[i] + A[u,:].B[i,:]`` on the device, ``A
    [n_users, kpad]``, ``B [n_items, kpad]``, ``c`` a device scalar: what every ``rfm_pair_*`` entry
    takes, in the order it takes it (``operands`` builds one)."""
    rt: Runtime
    A: object
    LU: object
    B: object
    LI: object
    c: object
    n_factors: int

    @property
    def n_users(self) -> int:
        return int(self.A.shape[0])

    @property
    def n_items(self) -> int:
        return int(self.B.shape[0])

    def pair_args(self, ids, n_sel: int) -> tuple:
        """The leading arguments of a ``rfm_pair_*`` call; ``ids``: device user ids, None = every user."""
        return (self.rt.ctx, self.A.data_ptr(), self.LU.data_ptr(), self.n_users,
                None if ids is None else ids.data_ptr(), n_sel, self.B.data_ptr(), self.LI.data_ptr(),
                self.n_items, self.n_factors, self.c.data_ptr())


def excl_args(excl) -> tuple:
    """The two exclusion pointers of a ``rfm_pair_*`` call for device lists ``excl`` (or None)."""
    return (None, None) if excl is None else (excl[0].data_ptr(), excl[1].data_ptr())


def side_sums(rt: Runtime, X: DeviceCSR, w, V, n_features: int, n_factors: int, A=None, L=None):
    """``(A [n, kpad], L [n])`` of a side matrix for ``w``, ``V`` (device tensors), into ``A``, ``L`` if given."""
    torch = __import__("torch")
    n, kp = X.shape[0], pad4(n_factors)
    if A is None:
        A, L = rt.empty((n, kp), torch.float64), rt.empty((n,), torch.float64)
    elif tuple(A.shape) != (n, kp) or tuple(L.shape) != (n,):
        raise ValueError(f"side sums of {n} rows x {kp} into buffers of {tuple(A.shape)}, {tuple(L.shape)}")
    _lib.check(rt.lib.rfm_fm_side_sums(rt.ctx, X.indptr.data_ptr(), X.indices.data_ptr(), X.values.data_ptr(), n,
                                       w.data_ptr(), V.data_ptr(), n_features, n_factors, A.data_ptr(),
                                       L.data_ptr()))
    return A, L


def padded(rt: Runtime, M, n_factors: int, out=None):
    """A dense ``[n, k]`` device matrix as ``[n, kpad]`` (itself when ``k % 4 == 0``), into ``out`` if
    given: an earlier result, whose columns past k stay zero."""
    torch = __import__("torch")
    kp = pad4(n_factors)
    if kp == n_factors:
        return M
    if out is None:
        out = torch.zeros((M.shape[0], kp), dtype=torch.float64, device=rt.torch_device)
    elif tuple(out.shape) != (M.shape[0], kp):  # (an earlier result for other rows, new_users= among them)
        raise ValueError(f"{M.shape[0]} rows x {kp} into a buffer of {tuple(out.shape)}")
    out[:, :n_factors] = M
    return out


def catalogue_shape(model, sides=None) -> Tuple[int, int]:
    """``(n_users, n_items)`` of a model's catalogue, after the checks that need no device."""
    if hasattr(model, "n_features"):
        if not isinstance(sides, Sides):
            raise TypeError("sides must be a recommend.Sides")
        if sides.n_features != model.n_features:
            raise ValueError(f"sides have {sides.n_features} columns, model has {model.n_features}")
        return sides.n_users, sides.n_items
    if not hasattr(model, "b"):
        # the reference's global bias exists only after fit() (src/mf.py:84)
        raise AttributeError("'LogisticMatrixFactorization' object has no attribute 'b'")
    return int(model.n_users), int(model.n_items)


def grown_side_sums(rt: Runtime, model, folded, S=None, L=None):
    """``(sums [n_new, kpad], L [n_new])`` of the GROWN rows of an FM model's ``FoldedColumns`` -- each new
    row's feature entries and then its own id column with entry 1 -- from the side-sum kernel itself:
    the bits that ``append_columns`` and a ``Sides`` of the grown width (id columns last) give the same
    rows.  ``folded.A`` holds the same sums, but ``folded.L`` is ``l + omega + g . nu`` as the fold
    launch forms it, which rounds otherwise than the kernel's ``(lin + omega) + cross / 2``.  Only the
    columns the rows store are gathered (w, V rows of the model, then the folded ones): the kernel
    reads nothing else, and a column's number plays no part in the sums."""
    torch = __import__("torch")
    import scipy.sparse as sp

    X = folded.features
    n_new, kf = int(X.shape[0]), int(model.n_factors)
    cols = np.unique(X.indices)
    local = sp.csr_matrix((X.data, np.searchsorted(cols, X.indices), X.indptr), shape=(n_new, cols.size))
    G = sp.hstack([local, sp.identity(n_new, format="csr")]).tocsr()  # (canonical: the id column comes last)
    at = rt.upload(cols.astype(np.int64)) if cols.size else torch.zeros((0,), dtype=torch.int64, device=rt.torch_device)
    w = torch.cat([model.w.dev.index_select(0, at), folded.w])
    V = torch.cat([model.V.dev.index_select(0, at), folded.V])
    return side_sums(rt, DeviceCSR(rt, G), w, V, int(G.shape[1]), kf, S, L)


def _fm_side(rt: Runtime, model, X: DeviceCSR, folded, S, L, grown=False):
    """One side's ``(sums, L)`` of an FM model: a side-sum launch over ``X``, or the served operands of
    ``folded`` (``grown``: ``grown_side_sums`` of it, where it carries its rows' feature entries); into
    ``S, L`` (buffers of an earlier result) if given."""
    if folded is None:
        return side_sums(rt, X, model.w.dev, model.V.dev, model.n_features, int(model.n_factors), S, L)
    if grown and getattr(folded, "features", None) is not None and len(folded):
        if S is not None and (tuple(S.shape) != tuple(folded.A.shape) or tuple(L.shape) != tuple(folded.L.shape)):
            raise ValueError(f"folded operands of {tuple(folded.A.shape)} into a buffer of {tuple(S.shape)}")
        return grown_side_sums(rt, model, folded, S, L)
    if S is None:
        return folded.A, folded.L
    # refreshed in place, as every other buffer of `into`
    if tuple(S.shape) != tuple(folded.A.shape) or tuple(L.shape) != tuple(folded.L.shape):
        raise ValueError(f"folded operands of {tuple(folded.A.shape)} into a buffer of {tuple(S.shape)}")
    if S.data_ptr() != folded.A.data_ptr():
        S.copy_(folded.A)
        L.copy_(folded.L)
    return S, L


def operands(model, sides=None, into: Optional[Operands] = None, new_users=None, new_items=None) -> Operands:
    """The ``Operands`` of a model as it stands.  FM (``sides``: its ``Sides``): two side-sum
    launches per call.  MF: ``P, b_u, Q, b_i``, the uploaded ``b``, zero-padded copies of P, Q when
    ``n_factors % 4``.  ``into``: an earlier result for the same shapes, whose buffers are refreshed
    in place on the runtime's stream -- no allocation, no host wait; buffers of another shape (the
    operands of the model's own users as ``into`` of a call with ``new_users``, say) are a
    ``ValueError``.  ``new_users`` (MF): the
    ``FoldedRows`` of ``fold_in_users``, whose rows and biases stand in for ``P, b_u`` (DESIGN.md 8
    N13): the operands' users are then the folded rows, and the model is not touched.  ``new_users``
    (FM): the ``FoldedColumns`` of ``fold_in_users``, whose served operands ``A, L`` stand in for the
    user side sums -- one side-sum launch, for the items; with ``into`` they are
    copied into its user buffers.  ``new_items``: the same for the item side, under
    the same checks and ``into`` rules -- the ``FoldedRows`` of ``fold_in_items`` stand in for ``Q,
    b_i``, the ``FoldedColumns`` of an FM model's ``fold_in_items`` for the item side sums; the two
    may be given together.  The FM item side is served as the rows will be once they are appended:
    one side-sum launch over the grown rows (``grown_side_sums``), so that ``new_items=`` and
    ``append_columns`` with a ``Sides`` of the grown width give the same bytes; ``FoldedColumns``
    built without their rows' feature entries are served through ``A, L``.  Folded rows of the other
    side, and those of the other model class, are a ``TypeError`` (``folded_queries``)."""
    is_fm = hasattr(model, "n_features")
    for side, folded in (("user", new_users), ("item", new_items)):
        if folded is not None:
            folded_queries(model, side, folded)
    catalogue_shape(model, sides)
    rt, kf = model._rt, int(model.n_factors)
    _, A, LU, B, LI, c, _ = into or (None,) * 7
    if is_fm:
        XU, XI = sides.device(rt)
        A, LU = _fm_side(rt, model, XU, new_users, A, LU)
        B, LI = _fm_side(rt, model, XI, new_items, B, LI, grown=True)
        return Operands(rt, A, LU, B, LI, model.w0.dev, kf)
    b = float(model.b)
    if c is None:
        c = rt.upload(np.array([b], dtype=np.float64))
    elif c.holds != b:  # (a fit does not change b: no launch between its iterations)
        c.fill_(b)
    c.holds = b
    user_rows, user_bias = (model.P.dev, model.b_u.dev) if new_users is None else (new_users.rows, new_users.bias)
    item_rows, item_bias = (model.Q.dev, model.b_i.dev) if new_items is None else (new_items.rows, new_items.bias)
    return Operands(rt, padded(rt, user_rows, kf, A), user_bias, padded(rt, item_rows, kf, B), item_bias, c, kf)


def is_int(v) -> bool:  # an integer argument: a Python or NumPy integer, not a bool
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _id_array(a, what: str, n: int) -> np.ndarray:
    """``a`` (``what``: "users" / "items") as int64; ``ValueError`` unless 1-d integers inside 0 .. n-1."""
    a = np.asarray(a)
    if a.ndim != 1 or (a.size and not np.issubdtype(a.dtype, np.integer)):
        raise ValueError(f"{what} must be a 1-d array of integer ids")
    if a.size and (a.min() < 0 or a.max() >= n):
        raise ValueError(f"{'a user' if what == 'users' else 'an item'} id lies outside 0..{n - 1}")
    return a.astype(np.int64)


def _users(rt: Runtime, users, n_users: int, what: str = "users"):
    """``(device ids or None, n_sel)`` of a selection of query rows (``what``: "users" / "items")."""
    if users is None:
        return None, n_users
    ids = _id_array(users, what, n_users).astype(np.int32)
    return rt.upload(ids if ids.size else np.zeros(1, np.int32)), int(ids.shape[0])


def _exclusions(rt: Runtime, excl):
    """The checked host lists ``excl`` (``_host_exclusions``) on the device, or None."""
    if excl is None:
        return None
    return rt.upload(excl[0]), rt.upload(excl[1] if excl[1].size else np.zeros(1, np.int32))


def _host_exclusions(exclude, n_users: int, n_items: int):
    """``exclude``: scipy sparse matrix (row = user id, stored columns = items), ``(indptr, indices)``
    or None; the checked host arrays ``(indptr int64, items int32)``, items ascending per user, or None."""
    if exclude is None:
        return None
    if isinstance(exclude, (tuple, list)):
        indptr, items = (np.asarray(a) for a in exclude)
    else:
        E = exclude.tocsr()
        if E.shape != (n_users, n_items):
            raise ValueError(f"exclude has shape {E.shape}, expected {(n_users, n_items)}")
        if not E.has_canonical_format:
            E = E.copy()
            E.sum_duplicates()
        indptr, items = E.indptr, E.indices
    indptr = np.ascontiguousarray(indptr, dtype=np.int64)
    items = np.ascontiguousarray(items, dtype=np.int32)
    if (indptr.shape != (n_users + 1,) or indptr[0] != 0 or indptr[-1] != items.shape[0]
            or np.any(np.diff(indptr) < 0)):
        raise ValueError(f"exclude: indptr must have {n_users + 1} monotone entries spanning the items")
    if items.size:
        if items.min() < 0 or items.max() >= n_items:
            raise ValueError(f"exclude: an item id lies outside 0..{n_items - 1}")
        rising = np.diff(items) > 0
        rising[indptr[1:-1][(indptr[1:-1] > 0) & (indptr[1:-1] < items.shape[0])] - 1] = True
        if not rising.all():
            raise ValueError("exclude: the item ids of a user must be strictly ascending")
    return indptr, items


def score_pairs(rt: Runtime, A, LU, B, LI, c, n_factors: int, users=None) -> np.ndarray:
    """Probabilities of every (selected user, item) pair, ``float64 [n_sel, n_items]``."""
    torch = __import__("torch")
    ops = Operands(rt, A, LU, B, LI, c, n_factors)
    ids, n_sel = _users(rt, users, ops.n_users)
    out = rt.empty((n_sel, ops.n_items), torch.float64)
    _lib.check(rt.lib.rfm_pair_scores(*ops.pair_args(ids, n_sel), out.data_ptr()))
    rt.sync()
    return out.cpu().numpy()


def topk(rt: Runtime, A, LU, B, LI, c, n_factors: int, k: int, users=None, exclude=None):
    """``(items int32 [n_sel, k], scores float64 [n_sel, k])``: the k best items per selected user by
    logit (ties: higher item index first), scores = sigmoid(logit); fewer than k rankable items
    pads with item -1 / score NaN."""
    torch = __import__("torch")
    ops = Operands(rt, A, LU, B, LI, c, n_factors)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k={k} outside 1..{MAX_K}")
    ids, n_sel = _users(rt, users, ops.n_users)
    excl = _exclusions(rt, _host_exclusions(exclude, ops.n_users, ops.n_items))
    ws = rt.empty((topk_workspace_bytes(n_sel, ops.n_items, k),), torch.uint8)
    items = rt.empty((n_sel, k), torch.int32)
    scores = rt.empty((n_sel, k), torch.float64)
    _lib.check(rt.lib.rfm_pair_topk(*ops.pair_args(ids, n_sel), *excl_args(excl), k, ws.data_ptr(),
                                    items.data_ptr(), scores.data_ptr()))
    rt.sync()
    return items.cpu().numpy(), scores.cpu().numpy()


def ranks_workspace_bytes(n_sel_users: int, n_items: int, n_targets: int) -> int:
    """Bytes of workspace ``rfm_pair_ranks`` needs (host only)."""
    out = C.c_int64(0)
    _lib.check(_lib.load().rfm_pair_ranks_workspace(int(n_sel_users), int(n_items), int(n_targets), C.byref(out)))
    return int(out.value)


def users_indptr(users) -> Tuple[np.ndarray, np.ndarray]:
    """``(sel int32, indptr int64)``: the unique user ids ascending and, for sorted ``users``, their runs."""
    sel, counts = np.unique(users, return_counts=True)
    return sel.astype(np.int32), np.concatenate(([0], np.cumsum(counts))).astype(np.int64)


def group_pairs(users, items, n_users: int, n_items: int, what=("users", "items")):
    """(user, item) pairs in any order, repeats allowed, as ``rfm_pair_ranks`` takes them:
    ``(sel_users int32, tgt_indptr int64, tgt_items int32, order)`` -- the unique users ascending,
    the items of selected user s ascending in ``tgt_items[tgt_indptr[s]:tgt_indptr[s + 1]]``, and
    ``order`` with grouped target t = input pair ``order[t]``.  ``ValueError`` for anything but two
    equal-length 1-d integer arrays of ids inside their tables.  ``what``: what the two arrays hold,
    ``("items", "users")`` for the by-item direction, which groups by item."""
    users, items = _id_array(users, what[0], n_users), _id_array(items, what[1], n_items)
    if users.shape != items.shape:
        raise ValueError(f"{users.shape[0]} {what[0]} for {items.shape[0]} {what[1]}: the pairs need one of each")
    order = np.lexsort((items, users))
    sel, indptr = users_indptr(users)
    return sel, indptr, items[order].astype(np.int32), order


def _first_excluded_pair(users, items, excl, n_items: int):
    """Index of the first input pair that the host exclusion lists ``excl`` name, or None."""
    indptr, listed = excl
    keys = np.repeat(np.arange(indptr.shape[0] - 1, dtype=np.int64), np.diff(indptr)) * n_items + listed
    hit = np.flatnonzero(np.isin(np.asarray(users, dtype=np.int64) * n_items + np.asarray(items, dtype=np.int64), keys))
    return int(hit[0]) if hit.size else None


def enqueue_ranks(ops: Operands, sel, n_sel: int, excl, tgt_indptr, tgt_items, n_targets: int, ws, ranks, scores,
                  cand) -> None:
    """The rank passes enqueued (``rfm_pair_ranks_n``: the host knows the number of targets) on device tensors."""
    _lib.check(ops.rt.lib.rfm_pair_ranks_n(*ops.pair_args(sel, n_sel), *excl_args(excl), tgt_indptr.data_ptr(),
                                           tgt_items.data_ptr(), n_targets, ws.data_ptr(), ranks.data_ptr(),
                                           scores.data_ptr(), cand.data_ptr()))


def _rank_grouped(rt: Runtime, A, LU, B, LI, c, n_factors: int, sel, tgt_indptr, tgt_items, excl):
    """``(ranks [n_targets], scores [n_targets], candidates [n_sel])`` of grouped targets (``group_pairs``)."""
    torch = __import__("torch")
    ops = Operands(rt, A, LU, B, LI, c, n_factors)
    n_sel, n_tgt = int(sel.shape[0]), int(tgt_items.shape[0])
    if n_sel == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.float64), np.zeros(0, np.int32)
    ws = rt.empty((ranks_workspace_bytes(n_sel, ops.n_items, n_tgt),), torch.uint8)
    ranks, scores = rt.empty((n_tgt,), torch.int32), rt.empty((n_tgt,), torch.float64)
    cand = rt.empty((n_sel,), torch.int32)
    enqueue_ranks(ops, rt.upload(sel), n_sel, _exclusions(rt, excl), rt.upload(tgt_indptr), rt.upload(tgt_items),
                  n_tgt, ws, ranks, scores, cand)
    rt.sync()
    return ranks.cpu().numpy(), scores.cpu().numpy(), cand.cpu().numpy()


def rank_items(rt: Runtime, A, LU, B, LI, c, n_factors: int, users, items, exclude=None):
    """Where the pairs ``(users[n], items[n])`` land in their users' ranking of the whole catalogue
    (DESIGN.md 8 N6): ``(ranks int32 [n], scores float64 [n], candidates int32 [n])`` in input
    order.  ``ranks[p]`` = number of items the user could be shown (logit not NaN, not in the
    user's ``exclude`` list) that are better than ``items[p]`` under ``topk``'s order, so that
    ``rank_items`` of ``topk``'s r-th item is r; ``candidates[p]`` = how many such items the user
    has; scores = sigmoid(logit).  A pair that ``exclude`` lists is a ``ValueError``."""
    ops = Operands(rt, A, LU, B, LI, c, n_factors)
    sel, tgt_indptr, tgt_items, order = group_pairs(users, items, ops.n_users, ops.n_items)
    excl = _host_exclusions(exclude, ops.n_users, ops.n_items)
    if excl is not None:
        p = _first_excluded_pair(users, items, excl, ops.n_items)
        if p is not None:
            raise ValueError(f"pair {p} (user {int(np.asarray(users)[p])}, item {int(np.asarray(items)[p])}) "
                             f"is in the user's exclusion list: it has no rank")
    g_ranks, g_scores, g_cand = _rank_grouped(*ops, sel, tgt_indptr, tgt_items, excl)
    n = order.shape[0]
    ranks, scores, cand = np.empty(n, np.int32), np.empty(n, np.float64), np.empty(n, np.int32)
    ranks[order], scores[order] = g_ranks, g_scores
    cand[order] = np.repeat(g_cand, np.diff(tgt_indptr))
    return ranks, scores, cand


def order_workspace_bytes(n_sel_users: int, n_items: int, depth: int) -> Tuple[int, int]:
    """``(min, preferred)`` bytes of workspace for ``rfm_pair_order`` (host only): one block of 64
    users / every selected user in one block; ``ValueError`` unless ``depth >= 1``."""
    lo, hi = C.c_int64(0), C.c_int64(0)
    _lib.check(_lib.load().rfm_pair_order_workspace(int(n_sel_users), int(n_items), _depth(depth), C.byref(lo),
                                                    C.byref(hi)))
    return int(lo.value), int(hi.value)


def _depth(depth) -> int:
    if not is_int(depth):
        raise ValueError(f"depth must be an integer, got {depth!r}")
    if depth < 1:
        raise ValueError(f"depth={int(depth)}: the ranking depth must be at least 1")
    return int(depth)


def rank_catalogue(rt: Runtime, A, LU, B, LI, c, n_factors: int, depth: int, users=None, exclude=None,
                   workspace_bytes: Optional[int] = None):
    """Every selected user's ranking of the catalogue down to ``depth``:
    ``(items int32 [n_sel, depth], scores float64 [n_sel, depth], n_ranked int32 [n_sel])``.
    Column r holds the candidate (logit not NaN, not in the user's ``exclude`` list) at position r
    of ``topk``'s order -- logit descending, ties: higher item index first -- and its
    sigmoid(logit); a row with fewer than ``depth`` candidates pads with item -1 / score NaN, and
    ``n_ranked`` is the user's candidate count (``rank_items``' ``candidates``).  ``depth`` is any
    integer >= 1; ``depth >= n_items`` gives the full ordering.  The first ``min(depth, 64)``
    columns are ``topk``'s bytes, and ``rank_items`` of the r-th returned item is r.
    ``workspace_bytes``: device memory for the logits of a block of users (``order_workspace_bytes``;
    default: the preferred size, at most ``ORDER_WORKSPACE_BYTES``); the result does not depend on it."""
    items, scores, n_ranked = rank_catalogue_device(rt, A, LU, B, LI, c, n_factors, depth, users, exclude,
                                                    workspace_bytes)
    rt.sync()
    return items.cpu().numpy(), scores.cpu().numpy(), n_ranked.cpu().numpy()


def rank_catalogue_device(rt: Runtime, A, LU, B, LI, c, n_factors: int, depth: int, users=None, exclude=None,
                          workspace_bytes: Optional[int] = None):
    """``rank_catalogue`` left on the device: its checks, its ``rfm_pair_order`` call and its workspace
    rule, and the three results as device tensors ``(items [n_sel, depth], scores [n_sel, depth],
    n_ranked [n_sel])`` on the runtime's stream, without a host wait -- what ``diverse`` selects from."""
    torch = __import__("torch")
    ops = Operands(rt, A, LU, B, LI, c, n_factors)
    depth = _depth(depth)
    ids, n_sel = _users(rt, users, ops.n_users)
    excl = _exclusions(rt, _host_exclusions(exclude, ops.n_users, ops.n_items))
    if n_sel == 0:
        return rt.empty((0, depth), torch.int32), rt.empty((0, depth), torch.float64), rt.empty((0,), torch.int32)
    least, preferred = order_workspace_bytes(n_sel, ops.n_items, depth)
    if workspace_bytes is None:
        workspace_bytes = max(least, min(preferred, ORDER_WORKSPACE_BYTES))
    workspace_bytes = int(workspace_bytes)
    if workspace_bytes < least:
        raise ValueError(f"workspace_bytes={workspace_bytes} is less than one block of 64 users ({least} bytes)")
    ws = rt.empty((workspace_bytes,), torch.uint8)
    items = rt.empty((n_sel, depth), torch.int32)
    scores = rt.empty((n_sel, depth), torch.float64)
    n_ranked = rt.empty((n_sel,), torch.int32)
    _lib.check(rt.lib.rfm_pair_order(*ops.pair_args(ids, n_sel), *excl_args(excl), depth, ws.data_ptr(),
                                     workspace_bytes, items.data_ptr(), scores.data_ptr(), n_ranked.data_ptr()))
    return items, scores, n_ranked


# ---------------------------------------------------------------------------
# the item -> users direction
# ---------------------------------------------------------------------------
def by_item(ops: Operands, entry: str, item_ids, n_sel: int, excl, *tail) -> None:
    """``rfm_pair_<entry>_by_item`` enqueued on ``ops``: the one place where an ``Operands`` becomes a
    call of the by-item direction.  The operand arguments are ``pair_args``' as they stand (the ABI
    exchanges the tables itself and keeps the user's side term first in the sum); ``item_ids``:
    device item ids, None = every item; ``excl``: device lists BY ITEM (``transposed_exclusions``)."""
    call = getattr(ops.rt.lib, f"rfm_pair_{entry}_by_item")
    _lib.check(call(*ops.pair_args(item_ids, n_sel), *excl_args(excl), *tail))


def transposed_exclusions(excl, n_items: int):
    """The checked host lists ``excl`` of ``_host_exclusions`` (by user, items ascending) as the lists
    by item that the by-item entries take: ``(indptr int64 [n_items + 1], users int32)``, the user
    ids of an item ascending -- a stable sort by item keeps the users in the order they come in,
    which is ascending.  None stays None."""
    if excl is None:
        return None
    indptr, items = excl
    users = np.repeat(np.arange(indptr.shape[0] - 1, dtype=np.int32), np.diff(indptr))
    t_indptr = np.concatenate(([0], np.cumsum(np.bincount(items, minlength=n_items)))).astype(np.int64)
    return t_indptr, users[np.argsort(items, kind="stable")]


def topk_users(rt: Runtime, A, LU, B, LI, c, n_factors: int, k: int, items=None, exclude=None):
    """``topk`` in the other direction: ``(users int32 [n_sel, k], scores float64 [n_sel, k])``, the k
    best users per selected item by logit (ties: higher user index first), scores = sigmoid(logit)
    with the bytes ``topk`` gives the same pair; fewer than k rankable users pads with user -1 /
    score NaN.  ``exclude``: what ``topk`` takes, by USER id -- one matrix serves both directions."""
    torch = __import__("torch")
    ops = Operands(rt, A, LU, B, LI, c, n_factors)
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k={k} outside 1..{MAX_K}")
    ids, n_sel = _users(rt, items, ops.n_items, "items")
    excl = _exclusions(rt, transposed_exclusions(_host_exclusions(exclude, ops.n_users, ops.n_items), ops.n_items))
    ws = rt.empty((topk_workspace_bytes(n_sel, ops.n_users, k),), torch.uint8)
    users = rt.empty((n_sel, k), torch.int32)
    scores = rt.empty((n_sel, k), torch.float64)
    by_item(ops, "topk", ids, n_sel, excl, k, 0, ws.data_ptr(), users.data_ptr(), scores.data_ptr())
    rt.sync()
    return users.cpu().numpy(), scores.cpu().numpy()


def rank_users(rt: Runtime, A, LU, B, LI, c, n_factors: int, items, users, exclude=None):
    """``rank_items`` in the other direction: where user ``users[p]`` stands among all users in item
    ``items[p]``'s ranking -- ``(ranks int32 [n], scores float64 [n], candidates int32 [n])`` in input
    order, 0-based, ``candidates[p]`` = the users the item could be shown to (logit not NaN, the
    pair not in ``exclude``, which is by USER id as everywhere).  ``rank_users`` of ``topk_users``'
    r-th user is r.  A pair that ``exclude`` lists is a ``ValueError``."""
    torch = __import__("torch")
    ops = Operands(rt, A, LU, B, LI, c, n_factors)
    sel, tgt_indptr, tgt_users, order = group_pairs(items, users, ops.n_items, ops.n_users, ("items", "users"))
    excl = _host_exclusions(exclude, ops.n_users, ops.n_items)
    if excl is not None:
        p = _first_excluded_pair(users, items, excl, ops.n_items)
        if p is not None:
            raise ValueError(f"pair {p} (item {int(np.asarray(items)[p])}, user {int(np.asarray(users)[p])}) "
                             f"is in the user's exclusion list: it has no rank")
    n = order.shape[0]
    ranks, scores, cand = np.empty(n, np.int32), np.empty(n, np.float64), np.empty(n, np.int32)
    n_sel = int(sel.shape[0])
    if n_sel == 0:
        return ranks, scores, cand
    ws = rt.empty((ranks_workspace_bytes(n_sel, ops.n_users, n),), torch.uint8)
    g_ranks, g_scores = rt.empty((n,), torch.int32), rt.empty((n,), torch.float64)
    g_cand = rt.empty((n_sel,), torch.int32)
    d_sel, d_indptr, d_users = rt.upload(sel), rt.upload(tgt_indptr), rt.upload(tgt_users)
    d_excl = _exclusions(rt, transposed_exclusions(excl, ops.n_items))
    by_item(ops, "ranks", d_sel, n_sel, d_excl, d_indptr.data_ptr(), d_users.data_ptr(), n, ws.data_ptr(),
            g_ranks.data_ptr(), g_scores.data_ptr(), g_cand.data_ptr())
    rt.sync()
    ranks[order], scores[order] = g_ranks.cpu().numpy(), g_scores.cpu().numpy()
    cand[order] = np.repeat(g_cand.cpu().numpy(), np.diff(tgt_indptr))
    return ranks, scores, cand


def rank_audience(rt: Runtime, A, LU, B, LI, c, n_factors: int, depth: int, items=None, exclude=None,
                  workspace_bytes: Optional[int] = None):
    """``rank_catalogue`` in the other direction: every selected item's ranking of the users down to
    ``depth`` (any integer >= 1; ``depth >= n_users``: all of them) -- ``(users int32 [n_sel, depth],
    scores float64 [n_sel, depth], n_ranked int32 [n_sel])``, short rows padded with user -1 / score
    NaN.  The first ``min(depth, 64)`` columns are ``topk_users``' bytes.  ``workspace_bytes``: as
    ``rank_catalogue`` takes it, for a block of items' rows of logits over the users."""
    torch = __import__("torch")
    ops = Operands(rt, A, LU, B, LI, c, n_factors)
    depth = _depth(depth)
    ids, n_sel = _users(rt, items, ops.n_items, "items")
    excl = _exclusions(rt, transposed_exclusions(_host_exclusions(exclude, ops.n_users, ops.n_items), ops.n_items))
    if n_sel == 0:
        return np.zeros((0, depth), np.int32), np.zeros((0, depth), np.float64), np.zeros(0, np.int32)
    least, preferred = order_workspace_bytes(n_sel, ops.n_users, depth)
    if workspace_bytes is None:
        workspace_bytes = max(least, min(preferred, ORDER_WORKSPACE_BYTES))
    workspace_bytes = int(workspace_bytes)
    if workspace_bytes < least:
        raise ValueError(f"workspace_bytes={workspace_bytes} is less than one block of 64 items ({least} bytes)")
    ws = rt.empty((workspace_bytes,), torch.uint8)
    users = rt.empty((n_sel, depth), torch.int32)
    scores = rt.empty((n_sel, depth), torch.float64)
    n_ranked = rt.empty((n_sel,), torch.int32)
    by_item(ops, "order", ids, n_sel, excl, depth, ws.data_ptr(), workspace_bytes, users.data_ptr(),
            scores.data_ptr(), n_ranked.data_ptr())
    rt.sync()
    return users.cpu().numpy(), scores.cpu().numpy(), n_ranked.cpu().numpy()


# ---------------------------------------------------------------------------
# nearest neighbours in factor space
# ---------------------------------------------------------------------------
METRICS = ("cosine", "dot")


def _table(M, n_factors: int):
    """``M`` if it is a table of rows of ``n_factors`` factors: float64 ``[n, k]`` or ``[n, kpad]``, contiguous."""
    torch = __import__("torch")
    if M.dim() != 2 or M.dtype != torch.float64 or not M.is_contiguous() or M.shape[0] < 1:
        raise ValueError("a table of rows must be a contiguous float64 matrix with at least one row")
    if int(M.shape[1]) not in (int(n_factors), pad4(n_factors)):
        raise ValueError(f"rows of {tuple(M.shape)} for {int(n_factors)} factors")
    return M


def normalised(rt: Runtime, M, n_factors: int):
    """``(rows [n, kpad], norms [n])`` of a device table ``M`` (``[n, k]`` or ``[n, kpad]``): every row
    divided by its Euclidean norm over the first ``n_factors`` columns, the padding zero
    (``rfm_rows_normalise``, whose fixed order include/rfm_neighbours.h states).  A row whose norm is zero,
    NaN or infinite comes out as NaN."""
    torch = __import__("torch")
    M, kf = _table(M, n_factors), int(n_factors)
    n = int(M.shape[0])
    out, norms = rt.empty((n, pad4(kf)), torch.float64), rt.empty((n,), torch.float64)
    _lib.check(rt.lib.rfm_rows_normalise(rt.ctx, M.data_ptr(), n, kf, int(M.shape[1]), out.data_ptr(),
                                         norms.data_ptr()))
    return out, norms


def _with_self(excl, n: int):
    """The checked host lists ``excl`` (or None) of ``n`` rows with every row's own id merged in."""
    own = np.arange(n, dtype=np.int64)
    if excl is None:
        return np.arange(n + 1, dtype=np.int64), own.astype(np.int32)
    indptr, items = excl
    rows = np.repeat(own, np.diff(indptr))
    missing = np.ones(n, dtype=bool)
    missing[rows[items == rows]] = False
    add = own[missing]
    rows, items = np.concatenate([rows, add]), np.concatenate([items.astype(np.int64), add])
    order = np.lexsort((items, rows))
    indptr = np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n)))).astype(np.int64)
    return indptr, items[order].astype(np.int32)


def check_neighbours(n_rows: int, k, ids=None, metric="cosine", exclude=None, include_self=False,
                     n_queries: Optional[int] = None, what: str = "items"):
    """The checks of ``neighbours`` that need no device -> ``(k, ids int32 or None, host exclusion
    lists or None)``.  ``n_queries``: the rows of a query table of its own, None = the queries are
    rows of the table itself, whose own ids are merged into the lists unless ``include_self``."""
    k = int(k)
    if not 1 <= k <= MAX_K:
        raise ValueError(f"k={k} outside 1..{MAX_K}")
    if metric not in METRICS:
        raise ValueError(f"metric {metric!r} is neither 'cosine' nor 'dot'")
    own = n_queries is None
    if include_self and not own:
        raise ValueError("include_self with rows of another table: they are not in the catalogue and have no self")
    n_q = int(n_rows) if own else int(n_queries)
    sel = None if ids is None else _id_array(ids, what, n_q).astype(np.int32)
    excl = _host_exclusions(exclude, n_q, int(n_rows))
    if own and not include_self:
        excl = _with_self(excl, int(n_rows))
    return k, sel, excl


def neighbours(rt: Runtime, R, n_factors: int, k: int, ids=None, metric="cosine", exclude=None, include_self=False,
               queries=None, what: str = "items"):
    """The ``k`` (1..64) nearest rows of the device table ``R`` for every query:
    ``(ids int32 [n, k], values float64 [n, k])``, best first under ``topk``'s total order (value
    descending, then id descending), short lists padded with id -1 / value NaN.  Similarity is in
    FACTOR SPACE only: biases and linear terms play no part.

    ``queries`` None: the queries are the rows ``ids`` of ``R`` (None = all; any order, repeats
    allowed), and a query never gets itself unless ``include_self``.  ``queries`` given: another
    table of the same factor count whose rows (``ids`` index them) are the queries; nothing of
    ``R`` is their self.  ``metric`` "cosine": both tables go through ``normalised`` (once when they
    are one buffer), the value is the cosine, and a row without a direction (norm zero, NaN or
    infinite) is nobody's neighbour and has an empty list; "dot": the rows as they are.
    ``exclude``: as ``topk`` takes it, by query row id, shape ``(queries, rows of R)``.
    ``what`` names the ids in an error message ("users" / "items")."""
    torch = __import__("torch")
    kf = int(n_factors)
    R = _table(R, kf)
    if queries is not None:
        _table(queries, kf)
    k, sel, excl = check_neighbours(R.shape[0], k, ids, metric, exclude, include_self,
                                    None if queries is None else queries.shape[0], what)
    n_q = int((R if queries is None else queries).shape[0])
    n_sel = n_q if sel is None else int(sel.shape[0])
    if n_sel == 0:
        return np.zeros((0, k), np.int32), np.zeros((0, k), np.float64)
    if metric == "cosine":
        rows = lambda M: normalised(rt, M, kf)[0]  # noqa: E731
    else:
        rows = lambda M: M if M.shape[1] == pad4(kf) else padded(rt, M, kf)  # noqa: E731
    B = rows(R)
    same = queries is None or (queries.data_ptr() == R.data_ptr() and queries.shape == R.shape)
    A = B if same else rows(queries)
    zero = torch.zeros((max(n_q, int(R.shape[0])),), dtype=torch.float64, device=rt.torch_device)
    ops = Operands(rt, A, zero, B, zero, zero, kf)
    d_ids, d_excl = None if sel is None else rt.upload(sel), _exclusions(rt, excl)
    ws = rt.empty((topk_workspace_bytes(n_sel, ops.n_items, k),), torch.uint8)
    out_ids, values = rt.empty((n_sel, k), torch.int32), rt.empty((n_sel, k), torch.float64)
    _lib.check(rt.lib.rfm_pair_topk_raw(*ops.pair_args(d_ids, n_sel), *excl_args(d_excl), k, ws.data_ptr(),
                                        out_ids.data_ptr(), values.data_ptr()))
    rt.sync()
    return out_ids.cpu().numpy(), values.cpu().numpy()


def folded_queries(model, side: str, folded):
    """The query table of ``new_items`` / ``new_users`` (``side``: "item" / "user") of a similarity
    call: the folded rows of the model's own ``fold_in_<side>s``.  The other side's rows and the
    other model class's are a ``TypeError``, another factor count a ``ValueError``, as in ``operands``."""
    kf = int(model.n_factors)
    if hasattr(model, "n_features"):
        if getattr(folded, "side", None) != side or not hasattr(folded, "A"):
            raise TypeError(f"new_{side}s of an FM model takes the FoldedColumns of its fold_in_{side}s; rows "
                            "that are served from their features alone go into its recommend.Sides")
        if tuple(folded.A.shape[1:]) != (pad4(kf),):
            raise ValueError(f"folded operands of {tuple(folded.A.shape)} for a model of {kf} factors")
        return folded.A
    if getattr(folded, "side", None) != side or not hasattr(folded, "rows"):
        raise TypeError(f"new_{side}s takes the FoldedRows of fold_in_{side}s")
    if tuple(folded.rows.shape[1:]) != (kf,):
        raise ValueError(f"folded rows of {tuple(folded.rows.shape)} for a model of {kf} factors")
    return folded.rows


def similar(model, side: str, k: int, ids=None, metric="cosine", exclude=None, include_self=False, new_rows=None,
            sides=None):
    """``similar_items`` / ``similar_users`` of both model classes (``side``: "item" / "user"):
    ``neighbours`` among the rows of Q / P (MF) or among the side sums b_i / a_u of ``sides`` (FM: one
    side-sum launch, for the side asked for).  ``new_rows``: folded rows of that side as the queries
    against the model's own rows.  Every argument is checked before the first launch."""
    item = side == "item"
    n_rows = catalogue_shape(model, sides)[item]
    queries = None if new_rows is None else folded_queries(model, side, new_rows)
    request = (k, ids, metric, exclude, include_self)
    check_neighbours(n_rows, *request, None if queries is None else int(queries.shape[0]), side + "s")
    rt, kf = model._rt, int(model.n_factors)
    if hasattr(model, "n_features"):
        R, _ = side_sums(rt, sides.device(rt)[item], model.w.dev, model.V.dev, model.n_features, kf)
    else:
        R = (model.P, model.Q)[item].dev
    return neighbours(rt, R, kf, *request, queries, side + "s")


# ---------------------------------------------------------------------------
# diversified re-ranking
# ---------------------------------------------------------------------------
MAX_DIVERSE_DEPTH = 1024


def check_diverse(n_items: int, k, depth=None, trade_off=0.5, metric="cosine", item_penalty=None):
    """The checks of ``diverse`` that need no device -> ``(k, depth, trade_off, penalty float64
    [n_items] or None)``.  ``depth`` None: ``min(n_items, max(64, 4 k))``; an explicit depth is clamped
    to ``n_items`` (``rank_catalogue``'s ``depth >= n_items`` is the full ordering) and must not
    exceed ``MAX_DIVERSE_DEPTH`` after that."""
    n_items = int(n_items)
    if not is_int(k) or not 1 <= k <= MAX_K:
        raise ValueError(f"k={k!r} outside 1..{MAX_K}")
    k = int(k)
    depth = min(n_items, max(64, 4 * k)) if depth is None else min(_depth(depth), n_items)
    if depth > MAX_DIVERSE_DEPTH:
        raise ValueError(f"depth={depth}: at most {MAX_DIVERSE_DEPTH} candidates are re-ranked")
    if k > depth:
        raise ValueError(f"k={k} picks from depth={depth} candidates")
    try:
        lam = float(trade_off)
    except (TypeError, ValueError):
        raise ValueError(f"trade_off must be a number in [0, 1], got {trade_off!r}") from None
    if not 0.0 <= lam <= 1.0:  # (false for a NaN)
        raise ValueError(f"trade_off={lam} outside [0, 1]")
    if metric not in METRICS:
        raise ValueError(f"metric {metric!r} is neither 'cosine' nor 'dot'")
    penalty = None
    if item_penalty is not None:
        penalty = np.ascontiguousarray(item_penalty, dtype=np.float64)
        if penalty.shape != (n_items,):
            raise ValueError(f"item_penalty has shape {penalty.shape}, expected {(n_items,)}")
        if np.isnan(penalty).any():
            raise ValueError("item_penalty holds a NaN")
    return k, depth, lam, penalty


def diversify(rt: Runtime, cand_items, cand_scores, R, n_factors: int, k: int, trade_off: float, item_penalty=None):
    """Greedy MMR among each row's candidates, one ``rfm_diverse_select`` launch: device tensors in
    (``cand_items`` int32 and ``cand_scores`` float64 ``[n_lists, depth]``, the item rows ``R [n_items,
    k or kpad]``, ``item_penalty`` float64 ``[n_items]`` or None), four host arrays out --
    ``(items int32, scores float64, values float64, pos int32)``, each ``[n_lists, k]``: the chosen
    items in the order they were chosen, their scores as given, the MMR value each was chosen at and
    its position among the candidates; a row that runs out of eligible candidates pads with item -1 /
    NaN / NaN / pos -1.  The arithmetic is the one include/rfm_diverse.h states."""
    torch = __import__("torch")
    R, kf = _table(R, n_factors), int(n_factors)
    if (cand_items.dim() != 2 or cand_items.shape != cand_scores.shape or cand_items.dtype != torch.int32
            or cand_scores.dtype != torch.float64 or not cand_items.is_contiguous() or not cand_scores.is_contiguous()):
        raise ValueError("candidates must be contiguous [n_lists, depth] tensors, items int32 and scores float64")
    n_lists, depth = (int(v) for v in cand_items.shape)
    if item_penalty is not None and (item_penalty.dtype != torch.float64 or tuple(item_penalty.shape) != (R.shape[0],)
                                     or not item_penalty.is_contiguous()):
        raise ValueError(f"item_penalty must be a float64 tensor of {int(R.shape[0])} items")
    if n_lists == 0:
        none = np.zeros((0, int(k)))
        return none.astype(np.int32), none, none.copy(), none.astype(np.int32)
    items, pos = rt.empty((n_lists, int(k)), torch.int32), rt.empty((n_lists, int(k)), torch.int32)
    scores, values = rt.empty((n_lists, int(k)), torch.float64), rt.empty((n_lists, int(k)), torch.float64)
    _lib.check(rt.lib.rfm_diverse_select(rt.ctx, cand_items.data_ptr(), cand_scores.data_ptr(), n_lists, depth, depth,
                                         R.data_ptr(), int(R.shape[0]), kf, int(R.shape[1]),
                                         None if item_penalty is None else item_penalty.data_ptr(), float(trade_off),
                                         int(k), items.data_ptr(), scores.data_ptr(), values.data_ptr(),
                                         pos.data_ptr()))
    rt.sync()
    return items.cpu().numpy(), scores.cpu().numpy(), values.cpu().numpy(), pos.cpu().numpy()


def diverse(model, sides, k, depth=None, trade_off=0.5, users=None, exclude=None, metric="cosine",
            item_penalty=None, new_users=None):
    """``recommend_diverse`` of both model classes: ``(items, scores, values)`` of ``diversify`` on each
    user's ``depth`` most relevant items (the device ranking of ``rank_catalogue``) and the item table
    -- the rows of ``Q`` (MF) or the item side sums ``b_i`` of ``sides`` (FM), through ``normalised``
    for ``metric="cosine"``, as they are for ``"dot"``.  ``new_users``: folded users, as in the other
    forward calls; the candidates change, the item table does not.  Every argument is checked before
    the first launch.

    ``trade_off=1`` without a penalty leaves nothing to trade against relevance, and the call is ``topk``:
    ``recommend(k)``'s lists, the values the scores.  The selection itself would agree wherever the
    scores in play are distinct doubles; it ranks by the PROBABILITY, which saturates to exactly 1.0 /
    0.0 where the logits still differ (the reason ``topk`` ranks by logit), and equal values go by item
    id.  At any other ``trade_off`` such saturated candidates do tie in relevance and go by id."""
    n_users, n_items = catalogue_shape(model, sides)
    if new_users is not None:
        n_users = int(folded_queries(model, "user", new_users).shape[0])
    k, depth, lam, penalty = check_diverse(n_items, k, depth, trade_off, metric, item_penalty)
    if users is not None:
        _id_array(users, "users", n_users)
    _host_exclusions(exclude, n_users, n_items)
    ops = operands(model, sides, new_users=new_users)
    rt, kf = ops.rt, ops.n_factors
    if lam == 1.0 and penalty is None:
        items, scores = topk(*ops, k, users, exclude)
        return items, scores, scores.copy()
    cand_items, cand_scores, _ = rank_catalogue_device(*ops, depth, users, exclude)
    R = normalised(rt, ops.B, kf)[0] if metric == "cosine" else ops.B  # (B is [n_items, kpad] already)
    return diversify(rt, cand_items, cand_scores, R, kf, k, lam, None if penalty is None else rt.upload(penalty))[:3]
