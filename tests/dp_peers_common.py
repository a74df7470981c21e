"""One real rank of ``rfm_fm_fit_dp`` and W - 1 emulated peers in one process (test_dp_ranks_host.py,
test_gpu_dp_ranks.py).

``rfm_transport`` hands the three collectives of the data-parallel fit to the caller, and the
library's public entry points can compute everything another rank would have sent.  So a world of 8
or 63 ranks needs neither 8 nor 63 processes: ``EmulatedPeers`` builds the transport of rank r of W
whose callbacks play every other rank -- single-threaded, no torch.distributed, no spawn.  Each
callback first checks what the real rank handed over (sizes, offsets and every byte of the message),
then writes what the peers answer.

The first half of this module is the bookkeeping, host only (NumPy): the bounds a shard must report,
the cuts of both all-to-all exchanges, the rank-ordered sum of an owner and the two roundings an
updated value may take.  Importing the module touches neither the GPU nor the package's library;
test_dp_ranks_host.py holds this half to tests/np_dp_engine.NumpyDpEngine and shows that every check
rejects its mutation.

What an updated value may be: with s the float64 sum of a column's records in rank order (plain
adds, the leader's first), ``fl(theta - fl(lr * s))`` or the correctly rounded ``theta - lr * s`` (a
fused multiply-add); nothing else, no tolerance."""
import ctypes as C
from fractions import Fraction

import numpy as np

import grad_forms_common as gf
from relevance_factorizationmachine_amd.dist import owner_ranges, shard_bounds

LD = np.longdouble


# --------------------------------------------------------------------------
# host bookkeeping
# --------------------------------------------------------------------------
def shard_columns(X, rows, hot_cols):
    """Columns a shard's record list names: those of its rows' entries and, when the shard is not
    empty, every hot column of the plan."""
    if len(rows) == 0:
        return np.zeros(0, dtype=np.int64)
    return np.union1d(np.unique(X[np.asarray(rows)].indices), np.asarray(hot_cols)).astype(np.int64)


def expected_bounds(cols, n, world):
    """Position of every owner range in the ascending column list ``cols``, and the total
    (world + 1 entries; the g_w0 record is not counted)."""
    lo = np.clip(owner_ranges(n, world).astype(np.int64), 0, n)
    return np.concatenate([np.searchsorted(cols, lo), [len(cols)]]).astype(np.int32)


def send_counts(bounds, rank):
    """Records rank ``rank`` sends to every owner: its list cut at its bounds, the g_w0 record to the
    last rank.  ``bounds``: [world][world + 1], g_w0 records not counted."""
    cnt = np.diff(np.asarray(bounds[rank], dtype=np.int64))
    cnt[-1] += 1
    return cnt


def recv_counts(bounds, rank):
    """Records owner ``rank`` receives from every rank (one more from each when it is the last)."""
    b = np.asarray(bounds, dtype=np.int64)
    cnt = b[:, rank + 1] - b[:, rank]
    return cnt + 1 if rank == b.shape[0] - 1 else cnt


def segment_pointers(bounds, rank):
    return np.concatenate([[0], np.cumsum(recv_counts(bounds, rank))]).astype(np.int64)


def output_offsets(bounds):
    """First record of every owner's block in the list of all updated rows (world + 1 entries)."""
    world = np.asarray(bounds).shape[0]
    return np.concatenate([[0], np.cumsum([recv_counts(bounds, o).sum() for o in range(world)])]).astype(np.int64)


def _same(name, got, want):
    got, want = np.asarray(got, dtype=np.int64), np.asarray(want, dtype=np.int64)
    assert np.array_equal(got, want), f"{name}: got {got.tolist()}, want {want.tolist()}"


def check_first_exchange(bounds, rank, wb, soff, sbytes, roff, rbytes):
    """The first all-to-all of an iteration: the rank's list leaves cut exactly at its bounds, what
    arrives lies back to back in rank order."""
    send, recv = send_counts(bounds, rank), recv_counts(bounds, rank)
    _same("sbytes", sbytes, send * wb)
    _same("soff", soff, (np.cumsum(send) - send) * wb)
    _same("rbytes", rbytes, recv * wb)
    _same("roff", roff, (np.cumsum(recv) - recv) * wb)


def check_second_exchange(bounds, rank, wb, soff, sbytes, roff, rbytes):
    """The second all-to-all: the owner's whole block to every peer, every owner's block to its place."""
    off = output_offsets(bounds)
    world = len(off) - 1
    _same("sbytes", sbytes, np.full(world, (off[rank + 1] - off[rank]) * wb))
    _same("soff", soff, np.full(world, off[rank] * wb))
    _same("rbytes", rbytes, np.diff(off) * wb)
    _same("roff", roff, off[:-1] * wb)


def rank_order_sums(segs):
    """``segs``: what every rank sent to one owner, in rank order ([m_s][k + 2] each).  Returns
    ``(leader, sums)``: column -> position of its first record in the concatenated list, and column
    -> the float64 sum of its records' values ([k + 1]) added in that order."""
    leader, sums, pos = {}, {}, 0
    for seg in segs:
        for rec in np.asarray(seg, dtype=np.float64):
            c = int(rec[0])
            if c in leader:
                sums[c] = sums[c] + rec[1:]
            else:
                leader[c], sums[c] = pos, 0.0 + rec[1:]
            pos += 1
    return leader, sums


def plain_update(theta, lr, s):
    """fl(theta - fl(lr * s))"""
    return np.asarray(theta, dtype=np.float64) - np.float64(lr) * np.asarray(s, dtype=np.float64)


def fused_update(theta, lr, s):
    """The correctly rounded theta - lr * s of one element."""
    return float(Fraction(float(theta)) - Fraction(float(lr)) * Fraction(float(s)))


def owner_block(segs, w0, w, V, lr, n, k):
    """The block an owner emits for ``segs`` with the plain rounding: [column, V_new, w_new] at a
    column's first record, column -1 (zeros behind it) at its others; [n, 0.., w0_new] for column n."""
    leader, sums = rank_order_sums(segs)
    total = sum(len(s) for s in segs)
    out = np.zeros((total, k + 2))
    out[:, 0] = -1.0
    for c, i in leader.items():
        out[i, 0] = c
        if c == n:
            out[i, k + 1] = plain_update(np.asarray(w0).reshape(-1)[0], lr, sums[c][k])
        else:
            out[i, 1:] = plain_update(np.concatenate([V[c], [w[c]]]), lr, sums[c])
    return out


def check_owner_block(block, segs, w0, w, V, lr, n, k, last, what="owner block"):
    """Every record of an owner's block: the column's first record in rank order carries the column
    and one of the two roundings of theta - lr * s in every value, the others carry -1.  Returns
    column -> leader record."""
    leader, sums = rank_order_sums(segs)
    total = sum(len(s) for s in segs)
    block = np.asarray(block, dtype=np.float64)
    assert block.shape == (total, k + 2), (what, block.shape, total)
    want_col = np.full(total, -1.0)
    for c, i in leader.items():
        assert 0 <= c < n or (last and c == n), f"{what}: column {c} outside the owner's reach"
        want_col[i] = c
    bad = np.flatnonzero(block[:, 0] != want_col)
    assert bad.size == 0, (f"{what}: column fields differ at positions {bad[:8].tolist()}: got "
                           f"{block[bad[:8], 0].tolist()}, want {want_col[bad[:8]].tolist()}")
    named = {}
    for c, i in leader.items():
        got = block[i, 1:]
        if c == n:
            theta = np.concatenate([np.zeros(k), [np.asarray(w0).reshape(-1)[0]]])
            s = np.concatenate([np.zeros(k), [sums[c][k]]])
        else:
            theta, s = np.concatenate([V[c], [w[c]]]), sums[c]
        assert np.isfinite(s).all() and np.isfinite(theta).all(), (what, c)
        plain = plain_update(theta, lr, s)
        for f in np.flatnonzero(~(got == plain)):
            fused = fused_update(theta[f], lr, s[f])
            assert got[f] == fused, (f"{what}: column {c} value {f}: got {got[f]!r}, the roundings of theta - lr * s "
                                     f"are {plain[f]!r} and {fused!r} (theta {theta[f]!r}, s {s[f]!r})")
        named[c] = block[i].copy()
    return named


def rank_order_dense(grads):
    """((g_0 + g_1) + g_2) + ... in float64."""
    acc = np.array(grads[0], dtype=np.float64, copy=True)
    for g in grads[1:]:
        acc = acc + g
    return acc


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def assert_bits(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(bits(got).reshape(-1) != bits(want).reshape(-1))
    assert bad.size == 0, f"{what}: {bad.size} of {got.size} values differ in their bits, first at {bad[:4].tolist()}"


def global_oracle(log, ids, w0, w, V):
    """gf.fm_gradients_ld of the rows ``ids`` on the columns they touch, spread over all columns
    (a column no row holds has gradient and magnitude zero)."""
    X = log["features"][np.asarray(ids)]
    cols = np.unique(X.indices)
    n, k = V.shape
    g0, gw, GV, (S0, Sw, SV) = gf.fm_gradients_ld(X[:, cols], log["labels"][ids], log["pscores"][ids], w0, w[cols],
                                                  V[cols])
    out = [np.zeros(n, dtype=LD), np.zeros((n, k), dtype=LD), np.zeros(n, dtype=LD), np.zeros((n, k), dtype=LD)]
    for full, part in zip(out, (gw, GV, Sw, SV)):
        full[cols] = part
    return g0, out[0], out[1], (S0, out[2], out[3])


# --------------------------------------------------------------------------
# the device side
# --------------------------------------------------------------------------
class GuardedParams:
    """(w0, w, V) on the device with gf.GUARD NaN rows behind w and V."""

    def __init__(self, rt, w0, w, V):
        self.rt = rt
        self.n, self.k = V.shape
        wg, Vg = np.full(self.n + gf.GUARD, np.nan), np.full((self.n + gf.GUARD, self.k), np.nan)
        wg[: self.n], Vg[: self.n] = w, V
        self.w0 = rt.upload(np.asarray(w0, dtype=np.float64).reshape(1))
        self.w, self.V = rt.upload(wg), rt.upload(Vg)

    def ptrs(self):
        return self.w0.data_ptr(), self.w.data_ptr(), self.V.data_ptr()

    def host(self):
        self.rt.sync()
        w0, w, V = self.w0.cpu().numpy().copy(), self.w.cpu().numpy(), self.V.cpu().numpy()
        assert np.isnan(w[self.n:]).all() and np.isnan(V[self.n:]).all(), "a guard row behind w or V was written"
        return w0, w[: self.n].copy(), V[: self.n].copy()


class PeerCase:
    """A log with the plan of the rank under test on the runtime's context, and the same plan once
    more -- same arguments -- on a second context with a stream of its own for the peers: a call made
    from inside a callback never shares plan or context scratch with the fit in flight."""

    def __init__(self, rt, log, k, max_batch, hot):
        import torch
        from relevance_factorizationmachine_amd.runtime import Runtime
        self.rt, self.log, self.k, self.hot, self.max_batch = rt, log, k, hot, max_batch
        self.dev = gf.DeviceLog(rt, log, k, max_batch, hot)
        rt.sync()
        self.aux_stream = torch.cuda.Stream(device=rt.torch_device)
        with torch.cuda.stream(self.aux_stream):
            self.aux_rt = Runtime(rt.device)
            self.aux = gf.DeviceLog(self.aux_rt, log, k, max_batch, hot)
            self.aux_rt.sync()
        self.n = self.dev.n
        self.hot_cols = self.dev.plan.hot_columns()
        assert np.array_equal(self.hot_cols, self.aux.plan.hot_columns())
        assert self.dev.plan.layout() == self.aux.plan.layout()
        self.fixed = gf.fixed_order(k, hot)

    def on_aux(self):
        import torch
        return torch.cuda.stream(self.aux_stream)

    def close(self):
        self.rt.sync()
        self.aux_rt.sync()
        self.dev.close()
        self.aux.close()


class EmulatedPeers:
    """The transport of rank ``rank`` of ``world`` for ONE call of rfm_fm_fit_dp on ``case``.

    ids: [n_iters][global_batch] row ids.  mode: "rows" or "dense".  inject: (column, rank a, rank b)
    -- peer a's record of that column becomes 1e16 in every value and peer b's -1e16 (the oracle then
    does not apply).  tamper(table): edits the gathered bounds [world][n_iters][world + 1] before they
    are handed to the rank; the emulation then follows the edited table and compares no message with
    the truth (``strict`` False), only that nothing moves more records than exist.  fail: (collective
    name, call index) whose callback returns 1 at once.  loss_answer: the vector the loss all-reduce
    answers."""

    def __init__(self, case, world, rank, ids, params, lr, mode, inject=None, tamper=None, fail=None,
                 loss_answer=None, aux_bounds=True):
        from relevance_factorizationmachine_amd import _lib
        self.case, self.W, self.r, self.params, self.lr, self.mode = case, world, rank, params, float(lr), mode
        self.ids = np.ascontiguousarray(ids, dtype=np.int32)
        self.n_iters, self.B = self.ids.shape
        self.n, self.k = case.n, case.k
        self.wb = (self.k + 2) * 8
        self.inject, self.tamper, self.fail, self.loss_answer = inject, tamper, fail, loss_answer
        self.strict, self.aux_bounds = tamper is None, aux_bounds
        self.calls = {"all_gather": 0, "all_to_all": 0, "all_reduce_sum": 0}
        self.error = None
        self.theta = []       # the live replica at the start of every iteration, then the final one
        self.named = []       # rows mode: column -> leader record of every iteration, all owners
        self.expect = []      # dense mode: the replica rfm_fm_apply leaves after every iteration
        self.loss_seen = None
        self.ranges = owner_ranges(self.n, world)
        self.shards = [shard_bounds(self.B, world, s) for s in range(world)]
        self.table = None
        self._lib = _lib
        cbs = (_lib.TRANSPORT_ALL_GATHER(self._guard("all_gather", self._all_gather)),
               _lib.TRANSPORT_ALL_REDUCE(self._guard("all_reduce_sum", self._all_reduce)),
               _lib.TRANSPORT_ALL_TO_ALL(self._guard("all_to_all", self._all_to_all)))
        self.struct = _lib.Transport(None, world, rank, *cbs)
        self._keep = cbs

    # ---- plumbing -----------------------------------------------------------
    def _guard(self, name, fn):
        def wrapped(*args):
            index = self.calls[name]
            self.calls[name] += 1
            if self.fail == (name, index):
                return 1
            try:
                fn(index, *args[1:])
                return 0
            except BaseException as exc:  # noqa: BLE001 -- reported through the C return code
                if self.error is None:
                    self.error = exc
                return 1
        return wrapped

    def _d2h(self, ptr, nbytes, dtype):
        rt = self.case.rt
        buf = np.empty(int(nbytes), dtype=np.uint8)
        if nbytes:
            self._lib.check(rt.lib.rfm_copy_to_host(rt.ctx, buf.ctypes.data, ptr, int(nbytes)))
        return buf.view(dtype)

    def _h2d(self, ptr, arr):
        rt = self.case.rt
        arr = np.ascontiguousarray(arr)
        if arr.nbytes:
            self._lib.check(rt.lib.rfm_copy_to_device(rt.ctx, ptr, arr.ctypes.data, arr.nbytes))

    def shard_ids(self, s, it):
        lo, hi = self.shards[s]
        return self.ids[it, lo:hi]

    def _live(self):
        """The replica as it stands (the main stream synchronised first)."""
        self.case.rt.sync()
        return self.params.host()

    def _aux_records(self, s, it):
        """rfm_fm_grad_rows of shard s on the peers' plan at the live parameters -> (records with the
        g_w0 record appended, bounds)."""
        case = self.case
        with case.on_aux():
            rec = gf.grad_rows(case.aux, self.shard_ids(s, it), self.params, self.n, self.ranges)
        assert rec.count <= rec.cap
        rec.assert_rest_untouched()
        w0rec = np.zeros((1, self.k + 2))
        w0rec[0, 0], w0rec[0, self.k + 1] = self.n, rec.gw0
        return np.concatenate([rec.filled(), w0rec]), rec.bounds

    def _aux_reduce(self, rows, seg_ptr):
        import torch
        case = self.case
        out = np.zeros((len(rows), self.k + 2))
        if len(rows) == 0:
            return out
        with case.on_aux():
            rt = case.aux_rt
            d_rows, d_seg = rt.upload(rows), rt.upload(np.asarray(seg_ptr, dtype=np.int32))
            d_out = torch.zeros((len(rows) + gf.GUARD, self.k + 2), dtype=torch.float64, device=rt.torch_device)
            d_out[len(rows):] = float("nan")
            self._lib.check(rt.lib.rfm_fm_reduce_rows(rt.ctx, d_rows.data_ptr(), d_seg.data_ptr(), self.W, len(rows),
                                                      self.params.w.data_ptr(), self.params.V.data_ptr(), self.n,
                                                      self.k, self.lr, d_out.data_ptr()))
            rt.sync()
            res = d_out.cpu().numpy()
        assert np.isnan(res[len(rows):]).all(), "rfm_fm_reduce_rows wrote behind its output"
        return res[: len(rows)]

    # ---- all_gather: the bounds of every rank, every iteration -----------------
    def _all_gather(self, index, d_send, d_recv, nbytes):
        W, nb = self.W, self.W + 1
        assert self.mode == "rows" and index == 0, "an all-gather nobody expects"
        assert nbytes == self.n_iters * nb * 4, nbytes
        mine = self._d2h(d_send, nbytes, np.int32).reshape(self.n_iters, nb)
        X = self.case.log["features"]
        table = np.zeros((W, self.n_iters, nb), dtype=np.int32)
        for s in range(W):
            for it in range(self.n_iters):
                table[s, it] = expected_bounds(shard_columns(X, self.shard_ids(s, it), self.case.hot_cols), self.n, W)
        _same("the rank's bounds", mine, table[self.r])
        if self.aux_bounds:  # (the bounds do not depend on the parameters)
            for s in range(W):
                for it in range(self.n_iters):
                    _same(f"bounds of rank {s}, iteration {it}, by rfm_fm_grad_rows", self._aux_records(s, it)[1],
                          table[s, it])
        self.truth = table.copy()
        if self.tamper is not None:
            self.tamper(table)
        self.table = table
        self._h2d(d_recv, table)

    # ---- all_to_all -------------------------------------------------------------
    def _all_to_all(self, index, d_send, soff, sbytes, d_recv, roff, rbytes):
        assert self.mode == "rows" and self.table is not None and index < 2 * self.n_iters
        arrs = [np.array([a[p] for p in range(self.W)], dtype=np.int64) for a in (soff, sbytes, roff, rbytes)]
        if index % 2 == 0:
            self._records_to_owners(index // 2, d_send, d_recv, *arrs)
        else:
            self._rows_to_everybody(index // 2, d_send, d_recv, *arrs)

    def _records_to_owners(self, it, d_send, d_recv, soff, sbytes, roff, rbytes):
        W, r, k, n, wb = self.W, self.r, self.k, self.n, self.wb
        bounds = self.table[:, it, :]
        check_first_exchange(bounds, r, wb, soff, sbytes, roff, rbytes)
        planned = int(send_counts(bounds, r).sum())
        true_count = int(self.truth[r, it, W]) + 1
        assert planned <= true_count, "a transfer moves more records than exist"
        sent = self._d2h(d_send, planned * wb, np.float64).reshape(planned, k + 2).copy()
        self.theta.append(self._live())
        full = [self._aux_records(s, it)[0] for s in range(W)]
        if self.strict:
            self._check_sent(sent, full[r], it)
        for s in range(W):
            if s != r and self.shards[s][0] == self.shards[s][1]:  # an empty peer shard
                assert full[s].shape[0] == 1 and full[s][0, k + 1] == 0.0 and not np.signbit(full[s][0, k + 1])
        if self.inject is not None:
            col, a, b = self.inject
            for s, v in ((a, 1e16), (b, -1e16)):
                at = np.flatnonzero(full[s][:, 0] == col)
                assert s != r and at.size == 1, "the injected column is not in that peer's list"
                full[s][at[0], 1:] = v
            assert (sent[:, 0] == col).any(), "the shard does not touch the injected column"
        full[r] = sent
        cut = [np.concatenate([[0], np.cumsum(send_counts(bounds, s))]) for s in range(W)]
        self.segs = [[full[s][cut[s][o]: cut[s][o + 1]] for s in range(W)] for o in range(W)]  # [owner][source]
        for p in range(W):
            part = self.segs[r][p]
            assert part.nbytes == rbytes[p]
            self._h2d(d_recv + int(roff[p]), part)

    def _check_sent(self, sent, want, it):
        """The bytes the rank sent against the records of its shard from the peers' plan."""
        from conftest import rel_err
        k, n = self.k, self.n
        what = f"records of rank {self.r}, iteration {it}"
        assert sent.shape == want.shape, (what, sent.shape, want.shape)
        assert_bits(sent[:, 0], want[:, 0], f"{what}: columns")
        assert sent[-1, 0] == n and not sent[-1, 1: k + 1].any() and not np.signbit(sent[-1, 1: k + 1]).any(), what
        if self.shards[self.r][0] == self.shards[self.r][1]:
            assert sent.shape[0] == 1 and sent[0, k + 1] == 0.0 and not np.signbit(sent[0, k + 1]), what
        if self.case.fixed:
            assert_bits(sent, want, what)
        else:
            assert not np.isnan(sent).any(), what
            if sent.shape[0] > 1:
                assert rel_err(sent[:-1, 1: k + 1], want[:-1, 1: k + 1]) < 1e-13, what
                assert rel_err(sent[:-1, k + 1], want[:-1, k + 1]) < 1e-13, what
            g = want[-1, k + 1]
            assert abs(sent[-1, k + 1] - g) <= 1e-13 * max(abs(g), 1e-300), what

    def _rows_to_everybody(self, it, d_send, d_recv, soff, sbytes, roff, rbytes):
        W, r, k, n, wb = self.W, self.r, self.k, self.n, self.wb
        bounds = self.table[:, it, :]
        assert d_send == d_recv, "the second all-to-all is in place"
        check_second_exchange(bounds, r, wb, soff, sbytes, roff, rbytes)
        w0, w, V = self.theta[it]
        # every send block is read before any receive block is written (the same block for everybody)
        mine = self._d2h(d_send + int(soff[0]), int(sbytes[0]), np.float64).reshape(int(sbytes[0]) // wb, k + 2).copy()
        for p in range(1, W):
            assert soff[p] == soff[0] and sbytes[p] == sbytes[0]
        named = check_owner_block(mine, self.segs[r], w0, w, V, self.lr, n, k, r == W - 1,
                                  f"block of rank {r}, iteration {it}")
        for o in range(W):
            if o == r:
                continue
            segs = self.segs[o]
            rows = np.concatenate(segs)
            ptr = np.concatenate([[0], np.cumsum([len(s) for s in segs])])
            block = self._aux_reduce(rows, ptr)
            if o == W - 1:  # the public entry point emits -1 for the g_w0 records: the test's own sum
                at = np.flatnonzero(rows[:, 0] == n)
                if at.size:
                    s = rows[at[0], k + 1] + 0.0
                    for j in at[1:]:
                        s = s + rows[j, k + 1]
                    assert (block[at, 0] == -1.0).all()
                    block[at[0]] = 0.0
                    block[at[0], 0], block[at[0], k + 1] = n, plain_update(w0[0], self.lr, s)
            got = check_owner_block(block, segs, w0, w, V, self.lr, n, k, o == W - 1,
                                    f"block of peer {o}, iteration {it}")
            assert not (set(got) & set(named)), "two owners emit the same column"
            named.update(got)
            assert block.nbytes == rbytes[o]
            self._h2d(d_recv + int(roff[o]), block)
        self.named.append(named)

    # ---- all_reduce_sum -----------------------------------------------------------
    def _all_reduce(self, index, d_buf, count):
        n_dense = self.n_iters if self.mode == "dense" else 0
        if index < n_dense:
            return self._dense(index, d_buf, count)
        assert index == n_dense and self.loss_answer is not None, "an all-reduce nobody expects"
        assert count == 2 * self.n_iters, count
        self.loss_seen = self._d2h(d_buf, count * 8, np.float64).copy()
        self._h2d(d_buf, np.asarray(self.loss_answer, dtype=np.float64))

    def _dense(self, it, d_buf, count):
        from conftest import rel_err
        case, n, k, W, r = self.case, self.n, self.k, self.W, self.r
        assert count == n * (k + 1) + 1, count
        mine = self._d2h(d_buf, count * 8, np.float64).copy()
        self.theta.append(self._live())
        grads = []
        for s in range(W):
            ids = self.shard_ids(s, it)
            if len(ids) == 0:
                grads.append(np.zeros(count))
                continue
            with case.on_aux():
                grads.append(gf.dense_grad(case.aux, ids, self.params)[0])
        what = f"dense gradient of rank {r}, iteration {it}"
        if len(self.shard_ids(r, it)) == 0:
            assert not mine.any() and not np.signbit(mine).any(), f"{what}: an empty shard's buffer is not all zeros"
        elif case.fixed:
            assert_bits(mine, grads[r], what)
        else:
            assert not np.isnan(mine).any(), what
            for got, want in zip(gf.split_grad(mine, n, k)[:2], gf.split_grad(grads[r], n, k)[:2]):
                assert rel_err(got, want) < 1e-13, what
            assert abs(mine[-1] - grads[r][-1]) <= 1e-13 * max(abs(grads[r][-1]), 1e-300), what
        grads[r] = mine
        total = rank_order_dense(grads)
        self._h2d(d_buf, total)
        # what rfm_fm_apply makes of that sum on a copy of the live replica
        w0, w, V = self.theta[it]
        with case.on_aux():
            rt = case.aux_rt
            c = [rt.upload(a) for a in (w0, w, V)]
            d_g = rt.upload(total)
            self._lib.check(rt.lib.rfm_fm_apply(rt.ctx, c[0].data_ptr(), c[1].data_ptr(), c[2].data_ptr(),
                                                d_g.data_ptr(), n, k, self.lr))
            rt.sync()
            self.expect.append(tuple(t.cpu().numpy() for t in c))

    # ---- the call and what it must leave -------------------------------------------
    def run(self, val=None, want_losses=False, eps=1e-15):
        """One rfm_fm_fit_dp.  val: (DeviceCSR, y, p) of the validation log.  Returns the return code
        (the error text in ``self.message``); an exception of a callback is raised here."""
        import torch
        rt, case = self.case.rt, self.case
        self.d_ids = rt.upload(self.ids)
        nan = float("nan")
        self.out_train = torch.full((self.n_iters,), nan, dtype=torch.float64, device=rt.torch_device)
        self.out_val = torch.full((self.n_iters,), nan, dtype=torch.float64, device=rt.torch_device)
        vargs = (None, None, None, None, None, 0)
        if val is not None:
            csr, vy, vp = val
            vargs = (csr.indptr.data_ptr(), csr.indices.data_ptr(), csr.values.data_ptr(), vy.data_ptr(),
                     vp.data_ptr(), csr.shape[0])
        self.theta0 = self.params.host()
        rc = rt.lib.rfm_fm_fit_dp(rt.ctx, case.dev.plan.handle, C.byref(self.struct),
                                  {"dense": 0, "rows": 1}[self.mode], self.d_ids.data_ptr(), self.B, self.n_iters,
                                  *self.params.ptrs(), self.lr, *vargs, eps,
                                  self.out_train.data_ptr() if want_losses else None,
                                  self.out_val.data_ptr() if want_losses else None)
        self.message = self._lib.last_error() if rc != 0 else ""
        rt.sync()
        if self.error is not None:
            raise self.error
        self.rc = rc
        return rc

    def check_counts(self, losses=False):
        if self.mode == "rows":
            want = {"all_gather": 1, "all_to_all": 2 * self.n_iters, "all_reduce_sum": 1 if losses else 0}
        else:
            want = {"all_gather": 0, "all_to_all": 0, "all_reduce_sum": self.n_iters + (1 if losses else 0)}
        assert self.calls == want, (self.calls, want)

    def check_replica(self):
        """After a clean call: every transition of the replica, bit for bit.  Rows mode: a row a
        leader record names holds that record's bytes, every other row is unchanged; dense mode: the
        replica rfm_fm_apply leaves.  Guard rows stay NaN (GuardedParams.host)."""
        n, k = self.n, self.k
        final = self.params.host()
        states = self.theta + [final]
        assert len(states) == self.n_iters + 1
        for it in range(self.n_iters):
            (w0a, wa, Va), (w0b, wb_, Vb) = states[it], states[it + 1]
            what = f"iteration {it}"
            if self.mode == "dense":
                for got, want, name in zip((w0b, wb_, Vb), self.expect[it], ("w0", "w", "V")):
                    assert_bits(got, want, f"{what}: {name} against rfm_fm_apply")
                continue
            named = self.named[it]
            cols = np.array(sorted(c for c in named if c < n), dtype=np.int64)
            rec = np.array([named[c] for c in cols]).reshape(len(cols), k + 2)
            assert_bits(Vb[cols], rec[:, 1: k + 1], f"{what}: V rows named by a leader record")
            assert_bits(wb_[cols], rec[:, k + 1], f"{what}: w named by a leader record")
            assert n in named, f"{what}: nobody emitted the g_w0 record"
            assert_bits(w0b, named[n][k + 1: k + 2], f"{what}: w0")
            rest = np.setdiff1d(np.arange(n), cols)
            assert_bits(Vb[rest], Va[rest], f"{what}: V rows nobody named")
            assert_bits(wb_[rest], wa[rest], f"{what}: w nobody named")
        return final

    def oracle_excess(self):
        """Largest gf.step_excess ratio over the call's iterations: every step of the device against
        the long-double SGD step of the GLOBAL batch from the parameters the device held."""
        states = self.theta + [self.params.host()]
        worst = 0.0
        for it in range(self.n_iters):
            o = global_oracle(self.case.log, self.ids[it], *states[it])
            ex = gf.step_excess(states[it + 1], states[it], o, self.lr, self.B)
            worst = max(worst, max(float(np.max(e)) for e in ex))
        return worst
