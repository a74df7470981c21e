"""Shared by the tests of the item -> users direction (test_audience_host.py, test_gpu_audience.py;
csrc/rfm_pairs.hip's by-item form, include/rfm_audience.h): a NumPy float64
statement of the by-item tile on top of ``pair_tile_common.tile_statement`` that carries the
direction's own mutations, the host ranking of a logit matrix under the total order (logit
descending, then USER index descending), the checks the GPU tests go through, the case lists, and
thin wrappers of the three raw ABI calls.  Importing this module touches neither the GPU nor the
package under test.

Everything is stated for Zt [n_items, n_users], the logits of the FORWARD direction transposed:
row i is item i's view of the users.  The GPU tests harvest Z from ``rfm_pair_topk_raw`` and hold
the by-item entries to its bytes, so the lists are compared exactly, at every position, ties
included; the long-double oracle of pair_tile_common is held on top of that at its own tolerance,
which the transposition does not widen: the by-item logit is the same three adds and the same
chain of fused multiply-adds."""
import functools

import numpy as np

import pair_tile_common as pc

MUTATIONS = ("sides_exchanged", "lower_user_first", "excl_at_user_offsets")

# the bitwise case: items (queries) x users (candidates) over the tile edges, and the chunk classes
EDGE_SIZES, EDGE_FACTORS = pc.EDGE_SIZES, pc.EDGE_FACTORS
BITWISE_SHAPE = (65, 129)  # items x users
BITWISE_FACTORS = (1, 4, 33, 1024)
BITWISE_CASES = tuple((ni, nu, k) for k in EDGE_FACTORS for ni in EDGE_SIZES for nu in EDGE_SIZES) + \
    tuple(BITWISE_SHAPE + (k,) for k in BITWISE_FACTORS)
# the walks of pair_tile_common with the sides exchanged: a 70-ITEM table selected n_sel times, the
# users the long side -- n_users -> (user tiles, tiles per split, splits, tiles of the last split)
WALK_ITEMS = pc.WALK_USERS
WALK_SEL, WALK_FACTORS, WALK_K = pc.WALK_SEL, pc.WALK_FACTORS, pc.WALK_K
WALK_USERS = dict(pc.WALK_ITEMS)
WALK_EMPTY_SPLIT_ITEM, WALK_EMPTY_ITEM, WALK_NAN_USER = pc.WALK_EMPTY_SPLIT_USER, pc.WALK_EMPTY_USER, pc.WALK_NAN_ITEM
# the condition on the bitwise case's inputs (test_audience_host.py): the share of logits whose bytes
# the exchanged sum order changes
MIN_CHANGED_SHARE = 0.1


def operands(n_items, n_users, n_factors):
    """``pair_tile_common.operands`` named by this direction: (A [n_users, k], LU, B [n_items, k], LI, c)."""
    return pc.operands(n_users, n_items, n_factors)


# --------------------------------------------------------------------------
# the statement of the by-item tile
# --------------------------------------------------------------------------
def by_item_statement(A, LU, B, LI, c, item_ids=None, mutation=None):
    """Zt [selected items, n_users] in float64 as the by-item form orders it: the rows of the tile are
    items, so the accumulator is ``tile_statement``'s with the two tables exchanged (and no side
    term: 0.0 + acc is acc), and the side terms are added user first, ((c + LU[u]) + LI[i]) + acc.
    ``mutation`` "sides_exchanged": ((c + LI[i]) + LU[u]) + acc, what the forward form computes when
    a caller exchanges the tables."""
    assert mutation in (None, "sides_exchanged")
    acc = pc.tile_statement(B, np.zeros(len(LI)), A, np.zeros(len(LU)), 0.0, item_ids)
    rows = np.arange(len(LI)) if item_ids is None else np.asarray(item_ids, dtype=np.int64)
    lu, li = np.asarray(LU)[None, :], np.asarray(LI)[rows][:, None]
    if mutation == "sides_exchanged":
        return ((c + li) + lu) + acc
    return ((c + lu) + li) + acc


def changed_share(A, LU, B, LI, c):
    """The share of logits whose bytes differ between the two orders of the side terms."""
    a, b = by_item_statement(A, LU, B, LI, c), by_item_statement(A, LU, B, LI, c, mutation="sides_exchanged")
    return float(np.mean(a.view(np.uint64) != b.view(np.uint64)))


# --------------------------------------------------------------------------
# exclusion lists by item
# --------------------------------------------------------------------------
def transpose_lists(indptr, items, n_items):
    """Lists by user (items ascending) -> lists by item (users ascending): the plain statement, one
    pair after the other."""
    per_item = [[] for _ in range(n_items)]
    for u in range(len(indptr) - 1):
        for i in items[indptr[u]:indptr[u + 1]]:
            per_item[int(i)].append(u)
    t_indptr = np.concatenate([[0], np.cumsum([len(p) for p in per_item])]).astype(np.int64)
    return t_indptr, np.array([u for p in per_item for u in p], dtype=np.int32)


def excluded_mask(indptr, users, n_items, n_users, mutation=None):
    """Bool [n_items, n_users] of lists by item.  ``mutation`` "excl_at_user_offsets": candidate u is
    looked up in the list at USER u's offsets, indptr[u] .. indptr[u + 1] (nothing, past the indptr),
    not in item i's."""
    assert mutation in (None, "excl_at_user_offsets")
    M = np.zeros((n_items, n_users), dtype=bool)
    if mutation is None:
        M[np.repeat(np.arange(n_items), np.diff(indptr)), users] = True
        return M
    for u in range(min(n_users, n_items)):
        M[:, u] = u in users[indptr[u]:indptr[u + 1]].tolist()
    return M


# --------------------------------------------------------------------------
# the host ranking
# --------------------------------------------------------------------------
def ranking(z, excluded=None, mutation=None):
    """The candidates of one row (not NaN, not ``excluded``) best first: logit descending, then user
    index descending (``mutation`` "lower_user_first": ascending)."""
    assert mutation in (None, "lower_user_first")
    cand = ~np.isnan(z)
    if excluded is not None:
        cand &= ~np.asarray(excluded)
    idx = np.flatnonzero(cand)
    return idx[np.lexsort((idx if mutation else -idx, -z[idx]))]


def expected_lists(Zt, depth, sel=None, excluded=None, values_of=None, mutation=None):
    """``(users int32 [n, depth] padded with -1, values [n, depth] padded with NaN, n_ranked int32
    [n])`` of the selected items (None: all; an id outside the table has an empty list).
    ``excluded``: bool [n_items, n_users]; ``values_of``: the matrix the values are taken from
    (default Zt itself; the forward scores, for the entries that return sigmoids)."""
    n_items = Zt.shape[0]
    sel = np.arange(n_items) if sel is None else np.asarray(sel, dtype=np.int64)
    V = Zt if values_of is None else values_of
    users = np.full((len(sel), depth), -1, dtype=np.int32)
    values = np.full((len(sel), depth), np.nan)
    n_ranked = np.zeros(len(sel), dtype=np.int32)
    orders = {}  # (a selection names an item many times)
    for s, i in enumerate(sel.tolist()):
        if not 0 <= i < n_items:
            continue
        if i not in orders:
            orders[i] = ranking(Zt[i], None if excluded is None else excluded[i], mutation)
        order = orders[i]
        m = min(depth, len(order))
        users[s, :m], values[s, :m], n_ranked[s] = order[:m], V[i, order[:m]], len(order)
    return users, values, n_ranked


def expected_ranks(Zt, sel, tgt_indptr, tgt_users, excluded=None):
    """``(ranks int32 [n_targets], candidates int32 [n_sel])`` as include/rfm_audience.h states them: the
    candidates other than the target that are better than it, -1 for a NaN logit; a target that
    its item's list names is ranked against the candidates."""
    ranks = np.full(len(tgt_users), -1, dtype=np.int32)
    cand_of = np.zeros(len(sel), dtype=np.int32)
    known = {}
    for s, i in enumerate(np.asarray(sel).tolist()):
        if not 0 <= i < Zt.shape[0]:
            continue
        z = Zt[i]
        cand = ~np.isnan(z)
        if excluded is not None:
            cand &= ~excluded[i]
        cand_of[s] = cand.sum()
        for p in range(int(tgt_indptr[s]), int(tgt_indptr[s + 1])):
            u = int(tgt_users[p])
            if np.isnan(z[u]):
                continue
            if (i, u) not in known:
                idx = np.flatnonzero(cand & (np.arange(len(z)) != u))
                known[(i, u)] = int(((z[idx] > z[u]) | ((z[idx] == z[u]) & (idx > u))).sum())
            ranks[p] = known[(i, u)]
    return ranks, cand_of


def same_bytes(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_lists(users, values, Zt, depth, sel, excluded, what, n_ranked=None, values_of=None):
    """The lists are the host ranking of Zt, position by position, and every value has the bytes of
    Zt (of ``values_of``); the padding is user -1 / NaN."""
    want_users, want_values, want_n = expected_lists(Zt, depth, sel, excluded, values_of)
    assert users.dtype == np.int32 and values.dtype == np.float64, what
    np.testing.assert_array_equal(users, want_users, err_msg=what)
    ok = want_users >= 0
    assert np.isnan(values[~ok]).all(), what + ": a padded slot holds a value"
    differ = values[ok].view(np.uint64) != want_values[ok].view(np.uint64)
    assert not differ.any(), f"{what}: {int(differ.sum())} of {differ.size} values have other bytes"
    if n_ranked is not None:
        np.testing.assert_array_equal(n_ranked, want_n, err_msg=what)


def by_item_oracle(A, LU, B, LI, c):
    """``pair_tile_common.pair_oracle`` with items as the rows: z [n_items, n_users] and the tolerances."""
    return pc.pair_oracle(B, LI, A, LU, c)


def assert_against_oracle(users, values, o, depth, sel, excluded, what, raw):
    """The lists against the long-double oracle at pair_tile_common's tolerance: the oracle's order at
    every separated position, the same padding, every value within tol_z (``raw``) / tol_p."""
    sel = np.arange(o.z.shape[0]) if sel is None else np.asarray(sel)
    want, sep, _ = pc.oracle_lists(o, depth, users=sel, excluded=excluded)
    np.testing.assert_array_equal(users < 0, want < 0, err_msg=what)
    assert (users == want)[sep].all(), what + ": not the oracle's order at a separated position"
    ok = users >= 0
    rows = np.repeat(sel[:, None], depth, axis=1)[ok]
    ref, tol = (o.z, o.tol_z) if raw else (o.p, o.tol_p)
    return pc.assert_within(values[ok], ref[rows, users[ok]], tol[rows, users[ok]], what)


# --------------------------------------------------------------------------
# walks
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def walk_exclusions(n_users, tiles_per_split):
    """Bool [70 items, n_users]: item 3 loses every user of split 1, item 5 every user, the others a tenth."""
    M = pc.walk_exclusions(n_users, tiles_per_split)
    M.setflags(write=False)
    return M


# --------------------------------------------------------------------------
# the raw ABI calls (sentinels behind every output)
# --------------------------------------------------------------------------
def _upload(rt, A, LU, B, LI, c):
    dA, dB, dLU, dLI = (rt.upload(a) for a in (pc._padded(A), pc._padded(B), *pc._own(LU, LI)))
    return dA, dLU, dB, dLI, rt.upload(np.array([c], dtype=np.float64))


def _lead(rt, dev, n_users, ids, n_sel, n_items, k, excl):
    """The arguments every pair entry begins with, and the tensors that have to outlive the call."""
    dA, dLU, dB, dLI, dc = dev
    d_ids = None if ids is None else rt.upload(np.asarray(ids, dtype=np.int32))
    ex = None if excl is None else (rt.upload(np.asarray(excl[0], dtype=np.int64)),
                                    rt.upload(np.asarray(excl[1], dtype=np.int32) if len(excl[1]) else np.zeros(1, np.int32)))
    args = (rt.ctx, dA.data_ptr(), dLU.data_ptr(), n_users, None if d_ids is None else d_ids.data_ptr(), n_sel,
            dB.data_ptr(), dLI.data_ptr(), n_items, k, dc.data_ptr(), None if ex is None else ex[0].data_ptr(),
            None if ex is None else ex[1].data_ptr())
    return args, (dev, d_ids, ex)  # (the operands too: their memory must not be handed out again)


def _guarded(rt, n, dtype):
    return pc._filled(rt, (n + pc.GUARD,), dtype)


def _take(t, n, shape):
    a = t.cpu().numpy()
    sentinel = pc.SENTINEL_I32 if a.dtype == np.int32 else pc.SENTINEL_F64
    assert (a[n:] == sentinel).all(), "an element past the output was written"
    a = a[:n].reshape(shape)
    pc.assert_written(a)
    return a


def _workspace(rt, query, *sizes):
    import ctypes

    import torch
    from relevance_factorizationmachine_amd import _lib
    out = [ctypes.c_int64(0) for _ in range(2 if query == "rfm_pair_order_workspace" else 1)]
    _lib.check(getattr(rt.lib, query)(*(int(s) for s in sizes), *(ctypes.byref(o) for o in out)))
    n = int(out[-1].value)
    return torch.empty((n,), dtype=torch.uint8, device=rt.torch_device), n


def forward_topk_raw(rfm, A, LU, B, LI, c, K):
    """rfm_pair_topk_raw of every user -> (items [n_users, K], logits [n_users, K])."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    rt = rfm[3]
    n_users, n_items, k = A.shape[0], B.shape[0], A.shape[1]
    args, keep = _lead(rt, _upload(rt, A, LU, B, LI, c), n_users, None, n_users, n_items, k, None)
    ws, _ = _workspace(rt, "rfm_pair_topk_workspace", n_users, n_items, K)
    items, values = _guarded(rt, n_users * K, torch.int32), _guarded(rt, n_users * K, torch.float64)
    _lib.check(rt.lib.rfm_pair_topk_raw(*args, K, ws.data_ptr(), items.data_ptr(), values.data_ptr()))
    rt.sync()
    return _take(items, n_users * K, (n_users, K)), _take(values, n_users * K, (n_users, K))


def forward_logits(rfm, A, LU, B, LI, c):
    """Z [n_users, n_items]: the forward logits as ``rfm_pair_topk_raw`` returns them, harvested on
    64-item slices of the item table with k = 64 (a NaN logit is never ranked and stays NaN)."""
    Z = np.full((A.shape[0], B.shape[0]), np.nan)
    for i0 in range(0, B.shape[0], 64):
        items, values = forward_topk_raw(rfm, A, LU, B[i0:i0 + 64], LI[i0:i0 + 64], c, 64)
        rows, cols = np.nonzero(items >= 0)
        Z[rows, i0 + items[rows, cols]] = values[rows, cols]
    return Z


def topk_by_item(rfm, A, LU, B, LI, c, K, item_ids=None, excl=None, raw=True):
    """rfm_pair_topk_by_item -> (users [n_sel, K], values [n_sel, K]); ``excl``: lists by item."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    rt = rfm[3]
    n_users, n_items, k = A.shape[0], B.shape[0], A.shape[1]
    n_sel = n_items if item_ids is None else len(item_ids)
    args, keep = _lead(rt, _upload(rt, A, LU, B, LI, c), n_users, item_ids, n_sel, n_items, k, excl)
    ws, _ = _workspace(rt, "rfm_pair_topk_workspace", n_sel, n_users, K)
    users, values = _guarded(rt, n_sel * K, torch.int32), _guarded(rt, n_sel * K, torch.float64)
    _lib.check(rt.lib.rfm_pair_topk_by_item(*args, K, int(raw), ws.data_ptr(), users.data_ptr(), values.data_ptr()))
    rt.sync()
    return _take(users, n_sel * K, (n_sel, K)), _take(values, n_sel * K, (n_sel, K))


def ranks_by_item(rfm, A, LU, B, LI, c, tgt_indptr, tgt_users, item_ids=None, excl=None):
    """rfm_pair_ranks_by_item -> (ranks [n_targets], scores [n_targets], candidates [n_sel])."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    rt = rfm[3]
    n_users, n_items, k = A.shape[0], B.shape[0], A.shape[1]
    n_sel = n_items if item_ids is None else len(item_ids)
    n_tgt = len(tgt_users)
    args, keep = _lead(rt, _upload(rt, A, LU, B, LI, c), n_users, item_ids, n_sel, n_items, k, excl)
    d_indptr, d_tgt = rt.upload(np.asarray(tgt_indptr, dtype=np.int64)), rt.upload(np.asarray(tgt_users, dtype=np.int32))
    ws, _ = _workspace(rt, "rfm_pair_ranks_workspace", n_sel, n_users, n_tgt)
    ranks, scores = _guarded(rt, n_tgt, torch.int32), _guarded(rt, n_tgt, torch.float64)
    cand = _guarded(rt, n_sel, torch.int32)
    _lib.check(rt.lib.rfm_pair_ranks_by_item(*args, d_indptr.data_ptr(), d_tgt.data_ptr(), n_tgt, ws.data_ptr(),
                                             ranks.data_ptr(), scores.data_ptr(), cand.data_ptr()))
    rt.sync()
    return _take(ranks, n_tgt, (n_tgt,)), _take(scores, n_tgt, (n_tgt,)), _take(cand, n_sel, (n_sel,))


def order_by_item(rfm, A, LU, B, LI, c, depth, item_ids=None, excl=None):
    """rfm_pair_order_by_item -> (users [n_sel, depth], scores [n_sel, depth], n_ranked [n_sel])."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    rt = rfm[3]
    n_users, n_items, k = A.shape[0], B.shape[0], A.shape[1]
    n_sel = n_items if item_ids is None else len(item_ids)
    args, keep = _lead(rt, _upload(rt, A, LU, B, LI, c), n_users, item_ids, n_sel, n_items, k, excl)
    ws, ws_bytes = _workspace(rt, "rfm_pair_order_workspace", n_sel, n_users, depth)
    users, scores = _guarded(rt, n_sel * depth, torch.int32), _guarded(rt, n_sel * depth, torch.float64)
    n_ranked = _guarded(rt, n_sel, torch.int32)
    _lib.check(rt.lib.rfm_pair_order_by_item(*args, depth, ws.data_ptr(), ws_bytes, users.data_ptr(), scores.data_ptr(),
                                             n_ranked.data_ptr()))
    rt.sync()
    return (_take(users, n_sel * depth, (n_sel, depth)), _take(scores, n_sel * depth, (n_sel, depth)),
            _take(n_ranked, n_sel, (n_sel,)))
