"""One real rank of ``rfm_fm_fit_dp`` / ``rfm_fm_fit_dp_eval`` and W - 1 emulated peers in one process
(test_dp_ranks_host.py, test_gpu_dp_ranks.py, test_gpu_dp_eval_ranks.py).

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

With an evaluation description (``EvalArgs``) the call is rfm_fm_fit_dp_eval and the emulation plays
the peers of its one extra all-gather as well (test_gpu_dp_eval_ranks.py): the reference is the whole
evaluation log scored by rfm_fm_plan_forward and ranked by rfm_val_dcg on the peers' plan, the rank's
message must be its groups' rows of that table bit for bit with +0.0 everywhere else, and the peers
answer with their rows and NaN in every double that belongs to no group.  The host half of that --
``eval_block``, ``merge_blocks``, ``stable_rule_table`` -- is NumPy as well.

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
# host bookkeeping of the evaluator (rfm_fm_fit_dp_eval)
# --------------------------------------------------------------------------
class EvalLog:
    """An evaluation log in frame order with its grouping by user, as rfm_val_dcg takes it: ``order``
    (grouped position -> frame row, ascending user, frame order inside a user) and ``seg`` (row bounds
    of the groups in grouped order)."""

    def __init__(self, X, users, labels, pscores):
        self.X = X.tocsr()
        self.frame = {"user": np.asarray(users), "label": np.asarray(labels, dtype=np.float64),
                      "pscore": np.asarray(pscores, dtype=np.float64)}
        self.n_rows = self.X.shape[0]
        self.order = np.argsort(self.frame["user"], kind="stable").astype(np.int32)
        su = self.frame["user"][self.order]
        self.seg = np.concatenate([[0], np.flatnonzero(su[1:] != su[:-1]) + 1, [self.n_rows]]).astype(np.int32)
        self.n_seg = len(self.seg) - 1

    def with_ones(self):
        """The same log with every propensity 1 (what a null d_ev_pscores means)."""
        return EvalLog(self.X, self.frame["user"], self.frame["label"], np.ones(self.n_rows))


def eval_block(table, lo, hi, pad, stride, fill):
    """What rank with groups lo .. hi - 1 contributes to the evaluator's all-gather for one iteration:
    ``stride`` doubles, its groups' rows of ``table`` ([vals | counted | order-dependent], n_seg
    apart) at [u | pad + u | 2 pad + u], ``fill`` everywhere else."""
    table = np.asarray(table, dtype=np.float64)
    n_seg, m = table.shape[0] // 3, hi - lo
    assert table.shape == (3 * n_seg,) and 0 <= lo <= hi <= n_seg and m <= pad and stride >= 3 * pad
    out = np.full(stride, fill, dtype=np.float64)
    for part in range(3):
        out[part * pad: part * pad + m] = table[part * n_seg + lo: part * n_seg + hi]
    return out


def group_owner(group_lo, g):
    """The rank that owns group g: the LAST rank whose first group is <= g (ranks without groups
    repeat the start of the next owner)."""
    return int(np.searchsorted(np.asarray(group_lo)[:-1], g, side="right")) - 1


def merge_blocks(blocks, group_lo, pad, n_seg, owner=group_owner, parts=(0, 1, 2), shift=0):
    """The merge of the gathered blocks ([rank][stride], one iteration) into the table of the whole
    log, restated in NumPy: group g comes from its owner's block at [u | pad + u | 2 pad + u],
    u = g - group_lo[owner].  ``owner``, ``parts`` and ``shift`` are there for test_dp_ranks_host.py,
    which states wrong merges with them (another owner rule, part p read at parts[p] * pad, u + shift)."""
    out = np.empty(3 * n_seg, dtype=np.float64)
    for g in range(n_seg):
        r = owner(group_lo, g)
        u = g - int(group_lo[r]) + shift
        for p in range(3):
            out[p * n_seg + g] = blocks[r][parts[p] * pad + u]
    return out


def check_table(got, want, what):
    """A merged table against the reference table: every double, bit for bit (a NaN read from a
    peer's padding differs from any value a table holds)."""
    assert_bits(got, want, what)
    assert not np.isnan(np.asarray(got)).any(), f"{what}: a table holds no NaN"


def stable_rule_table(frame, scores, k):
    """Per user (ascending) the value, the counted flag and the order-dependent flag of IPS-DCG@k
    under the documented tie rule, from NumPy alone (eval_rule_common.py): among equal scores the
    later row ranks first; rows of different label or propensity that tie inside or across the first
    k ranks, or a NaN score, make a user order-dependent."""
    from eval_rule_common import order_dependent_users, stable_rule_dcg
    scores = np.asarray(scores, dtype=np.float64)
    vals, counted = stable_rule_dcg(frame, scores, frame["pscore"], k)
    return vals, counted, order_dependent_users(frame, scores, frame["pscore"], k)


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
        # (a factor count gf.CLASS_OF does not list: chunked once its lane units -- two adjacent factors
        # of an even count -- outnumber a wavefront's 64 lanes)
        self.fixed = gf.fixed_order(k, hot) if k in gf.CLASS_OF else (hot in (-1, -2) or -(-k // (2 - k % 2)) > 64)

    def on_aux(self):
        import torch
        return torch.cuda.stream(self.aux_stream)

    def close(self):
        self.rt.sync()
        self.aux_rt.sync()
        self.dev.close()
        self.aux.close()


class EvalCase:
    """An evaluation log (EvalLog) whole on the peers' context of a PeerCase, for the reference of
    rfm_fm_fit_dp_eval: its scores by rfm_fm_plan_forward on the peers' plan and their table by
    rfm_val_dcg -- the two public entries the evaluator is documented to equal bit for bit; neither
    runs the shard path, the merge or the means of many tables."""

    def __init__(self, case, elog):
        from relevance_factorizationmachine_amd.runtime import DeviceCSR
        assert elog.X.shape[1] == case.n, (elog.X.shape, case.n)
        self.case, self.log = case, elog
        with case.on_aux():
            rt = case.aux_rt
            self.csr = DeviceCSR(rt, elog.X)
            self.rows, self.seg = rt.upload(elog.order), rt.upload(elog.seg)
            self.labels = rt.upload(elog.frame["label"][elog.order])
            self.pscores = rt.upload(elog.frame["pscore"][elog.order])
            rt.sync()

    def reference(self, theta, k):
        """(scores in frame order, table [3 n_seg], out [2]) of the whole log at the replica ``theta``."""
        import torch
        from relevance_factorizationmachine_amd import _lib
        case, log = self.case, self.log
        with case.on_aux():
            rt, c = case.aux_rt, self.csr
            nan = float("nan")
            w0, w, V = (rt.upload(np.asarray(a, dtype=np.float64)) for a in theta)
            sc = torch.full((log.n_rows + gf.GUARD,), nan, dtype=torch.float64, device=rt.torch_device)
            tab = torch.full((3 * log.n_seg + gf.GUARD,), nan, dtype=torch.float64, device=rt.torch_device)
            out = torch.full((2,), nan, dtype=torch.float64, device=rt.torch_device)
            _lib.check(rt.lib.rfm_fm_plan_forward(rt.ctx, case.aux.plan.handle, c.indptr.data_ptr(),
                                                  c.indices.data_ptr(), c.values.data_ptr(), log.n_rows,
                                                  w0.data_ptr(), w.data_ptr(), V.data_ptr(), sc.data_ptr()))
            _lib.check(rt.lib.rfm_val_dcg(rt.ctx, sc.data_ptr(), self.seg.data_ptr(), self.rows.data_ptr(),
                                          self.labels.data_ptr(), self.pscores.data_ptr(), log.n_seg, k,
                                          tab.data_ptr(), out.data_ptr()))
            rt.sync()
            sc, tab, out = sc.cpu().numpy(), tab.cpu().numpy(), out.cpu().numpy()
        assert np.isnan(sc[log.n_rows:]).all() and np.isnan(tab[3 * log.n_seg:]).all(), "the reference wrote behind its outputs"
        assert not np.isnan(sc[: log.n_rows]).any() and not np.isnan(tab[: 3 * log.n_seg]).any()
        return sc[: log.n_rows], tab[: 3 * log.n_seg], out


class Slots:
    """``n`` slots of ``width`` doubles on the device, NaN-filled, with one more slot in front and one
    behind: ``ptr`` is slot 0, ``host()`` returns [n + 2][width] with slot s at index s + 1."""

    def __init__(self, rt, n, width):
        import torch
        self.rt, self.n, self.width = rt, n, width
        self.t = torch.full(((n + 2) * width,), float("nan"), dtype=torch.float64, device=rt.torch_device)
        self.ptr = self.t.data_ptr() + width * 8

    def host(self):
        self.rt.sync()
        return self.t.cpu().numpy().reshape(self.n + 2, self.width)


class EvalArgs:
    """The evaluation arguments of ONE rfm_fm_fit_dp_eval call of rank ``rank`` of ``world`` on the
    log of ``whole`` (an EvalCase): the shard's CSR, grouping, labels and propensities as the driver
    builds them (dist.DpEvalLoop), every output NaN-filled with a slot in front and one behind.

    pad / user_stride: above the smallest legal values when given.  scores_extra: columns of a score
    slot behind the shard's rows.  permute: the shard's CSR in a shuffled row order with d_rows mapping
    grouped position to CSR row.  ones: d_ev_pscores NULL (``whole`` then holds all-ones propensities).
    The fields may be edited before the call (the error cases do)."""

    def __init__(self, rt, whole, world, rank, k, n_iters, pad=None, user_stride=None, scores_extra=0, slot_first=0,
                 permute=None, ones=False):
        from relevance_factorizationmachine_amd.dist import group_shard_bounds
        from relevance_factorizationmachine_amd.runtime import DeviceCSR
        log = whole.log
        self.whole, self.world, self.rank, self.k, self.n_iters, self.slot_first = whole, world, rank, k, n_iters, slot_first
        self.group_lo = np.ascontiguousarray(group_shard_bounds(log.seg, world), dtype=np.int32)
        self.lo, self.hi = int(self.group_lo[rank]), int(self.group_lo[rank + 1])
        r0, r1 = int(log.seg[self.lo]), int(log.seg[self.hi])
        self.n_local, self.n_ev, self.n_ev_total, self.n_seg = self.hi - self.lo, r1 - r0, log.n_rows, log.n_seg
        self.pad = max(int(np.diff(self.group_lo).max()), 1) if pad is None else pad
        self.user_stride = 3 * self.pad if user_stride is None else user_stride
        self.scores_stride = max(self.n_ev + scores_extra, 1)
        frame_rows = log.order[r0:r1]  # grouped position of the shard -> frame row
        self.h_rows = None
        self.csr_frame_rows = frame_rows  # CSR row of the shard -> frame row
        if permute is not None:
            self.h_rows = np.random.default_rng(permute).permutation(self.n_ev).astype(np.int32)
            self.csr_frame_rows = np.empty_like(frame_rows)
            self.csr_frame_rows[self.h_rows] = frame_rows
        self.csr = DeviceCSR(rt, log.X[self.csr_frame_rows]) if self.n_ev else None
        self.rows = None if self.h_rows is None else rt.upload(self.h_rows)
        self.seg_ptr = rt.upload((log.seg[self.lo: self.hi + 1] - r0).astype(np.int32))
        self.labels = rt.upload(log.frame["label"][frame_rows] if self.n_ev else np.zeros(1))
        self.pscores = None if ones else rt.upload(log.frame["pscore"][frame_rows] if self.n_ev else np.ones(1))
        if ones:
            assert (log.frame["pscore"] == 1.0).all()
        n_slots = slot_first + n_iters + 1  # (one free slot behind the call's)
        self.scores = Slots(rt, n_slots, self.scores_stride)
        self.scratch = Slots(rt, n_slots, self.user_stride)
        self.full = Slots(rt, n_iters, max(3 * self.n_seg, 1))
        self.dcg = Slots(rt, n_iters, 2)

    def tail(self):
        """The arguments of rfm_fm_fit_dp_eval behind those of rfm_fm_fit_dp, in the header's order."""
        def p(t):
            return None if t is None else t.data_ptr()
        c = self.csr
        return [p(c and c.indptr), p(c and c.indices), p(c and c.values), self.n_ev, self.n_ev_total, p(self.seg_ptr),
                p(self.rows), p(self.labels), p(self.pscores), self.n_local, self.k, self.scores.ptr,
                self.scores_stride, self.scratch.ptr, self.user_stride, self.slot_first, self.group_lo.ctypes.data,
                self.pad, self.n_seg, self.full.ptr, self.dcg.ptr]

    def outputs_untouched(self):
        for name in ("scores", "scratch", "full", "dcg"):
            assert np.isnan(getattr(self, name).host()).all(), f"a refused call wrote to {name}"


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
        self.ev = None        # the EvalArgs of a rfm_fm_fit_dp_eval call (run(ev=...))
        self.ref = None       # ... its reference per iteration: (scores, table, out) of the whole log
        self.eval_sent = None  # ... what the rank handed to the evaluator's all-gather
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
        if self.ev is not None and index == (1 if self.mode == "rows" else 0):
            return self._eval_gather(d_send, d_recv, nbytes)
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

    # ---- all_gather of the evaluator: every rank's per-user tables of the whole call ----------
    def _eval_gather(self, d_send, d_recv, nbytes):
        ea, W, r, n_it = self.ev, self.W, self.r, self.n_iters
        done = (self.calls["all_to_all"] == 2 * n_it) if self.mode == "rows" else (self.calls["all_reduce_sum"] >= n_it)
        assert done and len(self.theta) == n_it, "the evaluator's all-gather comes after the last iteration"
        assert nbytes == n_it * ea.user_stride * 8, nbytes
        assert d_send == ea.scratch.ptr + ea.slot_first * ea.user_stride * 8, "the send pointer is not the call's first slot"
        # the replica after every iteration -> the whole log's scores, table and means on the peers' plan
        self.ref = [ea.whole.reference(theta, ea.k) for theta in self.theta[1:] + [self._live()]]
        mine = self._d2h(d_send, nbytes, np.float64).reshape(n_it, ea.user_stride).copy()
        lo, pad, stride = ea.group_lo, ea.pad, ea.user_stride
        recv = np.empty((W, n_it, stride))
        for it, (_, table, _) in enumerate(self.ref):
            assert_bits(mine[it], eval_block(table, lo[r], lo[r + 1], pad, stride, 0.0),
                        f"the evaluator's message of rank {r}, iteration {it} (its groups' rows of the reference "
                        "table, +0.0 everywhere else)")
            for s in range(W):  # a peer's padding is NaN: a merge or a mean that reads it shows
                recv[s, it] = mine[it] if s == r else eval_block(table, lo[s], lo[s + 1], pad, stride, np.nan)
            check_table(merge_blocks(recv[:, it], lo, pad, ea.n_seg), table, "the emulation's own merge")
        self.eval_sent = mine
        self._h2d(d_recv, recv)

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
    def run(self, val=None, want_losses=False, eps=1e-15, ev=None):
        """One rfm_fm_fit_dp, or with ``ev`` (an EvalArgs) one rfm_fm_fit_dp_eval.  val: (DeviceCSR, y,
        p) of the validation log.  Returns the return code (the error text in ``self.message``); an
        exception of a callback is raised here."""
        import torch
        rt, case = self.case.rt, self.case
        self.ev = ev
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
        entry = "rfm_fm_fit_dp" if ev is None else "rfm_fm_fit_dp_eval"
        args = [rt.ctx, case.dev.plan.handle, C.byref(self.struct), {"dense": 0, "rows": 1}[self.mode],
                self.d_ids.data_ptr(), self.B, self.n_iters, *self.params.ptrs(), self.lr, *vargs, eps,
                self.out_train.data_ptr() if want_losses else None, self.out_val.data_ptr() if want_losses else None]
        assert len(args) == len(self._lib.SIGNATURES["rfm_fm_fit_dp"])
        if ev is not None:
            args += ev.tail()
        sig = self._lib.SIGNATURES[entry]
        assert len(args) == len(sig), (entry, len(args), len(sig))
        for a, t in zip(args, sig):  # an integer argument is an integer, a pointer an address or NULL
            assert t is C.c_void_p or isinstance(a, float if t is C.c_double else int), (entry, a, t)
        rc = getattr(rt.lib, entry)(*args)
        self.message = self._lib.last_error() if rc != 0 else ""
        rt.sync()
        if self.error is not None:
            raise self.error
        self.rc = rc
        return rc

    def check_counts(self, losses=False, evaluator=False):
        if self.mode == "rows":
            want = {"all_gather": 1, "all_to_all": 2 * self.n_iters, "all_reduce_sum": 1 if losses else 0}
        else:
            want = {"all_gather": 0, "all_to_all": 0, "all_reduce_sum": self.n_iters + (1 if losses else 0)}
        assert evaluator == (self.ev is not None)
        want["all_gather"] += 1 if evaluator else 0
        assert self.calls == want, (self.calls, want)

    def check_evaluator(self):
        """After a clean rfm_fm_fit_dp_eval: scores, per-user slots, merged tables and means of every
        iteration against the reference of the whole log, bit for bit, every double around them still
        NaN; then the reference tables themselves against the tie rule restated in NumPy (flags exact,
        values and mean to 1e-12: float64 on both sides, the reference's term order per user, another
        fixed order over users -- the figure of tests/test_gpu_eval.py)."""
        ea, n_it = self.ev, self.n_iters
        assert self.ref is not None and len(self.ref) == n_it and self.eval_sent.shape == (n_it, ea.user_stride)
        first, n_seg = ea.slot_first + 1, ea.n_seg  # (slot s of a Slots sits at index s + 1)
        scores, scratch, full, dcg = ea.scores.host(), ea.scratch.host(), ea.full.host(), ea.dcg.host()
        for it, (ref_scores, table, out) in enumerate(self.ref):
            what = f"rank {self.r} of {self.W}, iteration {it}"
            assert_bits(scores[first + it, : ea.n_ev], ref_scores[ea.csr_frame_rows],
                        f"{what}: the shard's scores against the whole log's")
            assert np.isnan(scores[first + it, ea.n_ev:]).all(), f"{what}: a score column behind the shard's rows was written"
            assert_bits(scratch[first + it], self.eval_sent[it], f"{what}: the per-user slot against what was gathered")
            check_table(full[1 + it, : 3 * n_seg], table, f"{what}: d_full_out against rfm_val_dcg of the whole log")
            got = dcg[1 + it]
            assert np.isnan(got[0]) if np.isnan(out[0]) else bits(got[:1])[0] == bits(out[:1])[0], (what, got, out)
            assert bits(got[1:])[0] == bits(out[1:])[0], (what, got, out)
            # independent of device code: the tie rule in NumPy on the reference's scores
            vals, counted, dep = stable_rule_table(ea.whole.log.frame, ref_scores, ea.k)
            assert np.array_equal(table[n_seg: 2 * n_seg], counted.astype(np.float64)), f"{what}: counted flags"
            assert np.array_equal(table[2 * n_seg:], dep.astype(np.float64)), f"{what}: order-dependent flags"
            assert not table[:n_seg][~counted].any(), f"{what}: a user that does not count has a value"
            np.testing.assert_allclose(table[:n_seg][counted], vals[counted], rtol=1e-12, atol=0, err_msg=what)
            assert out[1] == dep.sum(), (what, out[1], dep.sum())
            if counted.any():
                mean = float(np.mean(vals[counted]))
                assert abs(out[0] - mean) <= 1e-12 * abs(mean), (what, out[0], mean)
            else:
                assert np.isnan(out[0]) and np.isnan(got[0]), (what, out, got)
        call = np.zeros(scores.shape[0], dtype=bool)
        call[first: first + n_it] = True
        assert np.isnan(scores[~call]).all(), "a score slot outside the call was written"
        assert np.isnan(scratch[~call]).all(), "a per-user slot outside the call was written"
        assert np.isnan(full[[0, -1]]).all() and np.isnan(full[1:-1, 3 * n_seg:]).all(), "d_full_out: written outside the tables"
        assert np.isnan(dcg[[0, -1]]).all(), "d_dcg_out: written outside the call's pairs"

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
