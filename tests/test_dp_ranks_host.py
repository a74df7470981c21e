"""The bookkeeping of the emulated-peer harness (dp_peers_common.py) on the CPU: its expected bounds,
exchange cuts, rank-ordered sums and rounding candidates against tests/np_dp_engine.NumpyDpEngine at
2, 8 and 63 ranks, and a mutation that every check of a message must reject; then the evaluator's
half: blocks and their merge against random tables cut by dist.group_shard_bounds, and the wrong
merges that the table comparison of test_gpu_dp_eval_ranks.py must reject.  No GPU."""
import types

import numpy as np
import pytest

import dp_peers_common as dp
import grad_forms_common as gf
from np_dp_engine import NumpyDpEngine
from relevance_factorizationmachine_amd.dist import owner_ranges, shard_bounds


def _engine(log, k, lr, B, W, r, theta, transport):
    model = types.SimpleNamespace(seed=3, n_factors=k, n_epochs=1, batch_size=B, lr=lr)
    eng = NumpyDpEngine(model, log, None, W, r, "rows", transport)
    eng.w0, eng.w, eng.V = (np.array(a, dtype=np.float64, copy=True) for a in theta)
    return eng


def _records(eng, rows, n, k):
    GV, gw, g0, cols = eng._grads(rows)
    rec = np.concatenate([cols[:, None].astype(np.float64), GV[cols], gw[cols, None]], axis=1)
    return np.concatenate([rec, [[float(n)] + [0.0] * k + [g0]]]), cols


class HostPeers:
    """The host transport of NumpyDpEngine for rank r: every other rank is computed here, and what the
    engine hands over is held to the harness's bookkeeping."""

    def __init__(self, log, k, lr, ids, W, r, theta):
        self.W, self.r, self.k, self.lr, self.theta = W, r, k, lr, theta
        X = log["features"]
        self.n = n = X.shape[1]
        self.wb = (k + 2) * 8
        helper = _engine(log, k, lr, len(ids), W, 0, theta, None)
        shards = [ids[slice(*shard_bounds(len(ids), W, s))] for s in range(W)]
        self.full = [_records(helper, rows, n, k)[0] for rows in shards]
        self.bounds = np.stack([dp.expected_bounds(dp.shard_columns(X, rows, []), n, W) for rows in shards])
        for s in range(W):  # the two statements of a shard's columns agree
            assert np.array_equal(self.full[s][:-1, 0], dp.shard_columns(X, shards[s], []))
        cut = [np.concatenate([[0], np.cumsum(dp.send_counts(self.bounds, s))]) for s in range(W)]
        self.segs = [[self.full[s][cut[s][o]: cut[s][o + 1]] for s in range(W)] for o in range(W)]
        self.blocks = [dp.owner_block(self.segs[o], *theta, lr, n, k) for o in range(W)]
        self.step = 0

    def all_gather_host(self, arr):
        W, r = self.W, self.r
        if self.step == 0:
            want = self.bounds.astype(np.int64)
            want[:, W] += 1  # the engine counts its g_w0 record
            assert np.array_equal(arr, want[r])
            self.step = 1
            return want
        assert self.step == 2
        live = [int((b[:, 0] >= 0).sum()) * self.wb for b in self.blocks]
        assert int(arr[0]) == live[r]
        self.step = 3
        return np.array(live, dtype=np.int64).reshape(W, 1)

    def all_to_all_host(self, send, recv_bytes):
        W, r, wb, k = self.W, self.r, self.wb, self.k
        if self.step == 1:
            soff = np.concatenate([[0], np.cumsum([len(s) for s in send])])[:-1]
            seg = dp.segment_pointers(self.bounds, r)
            dp.check_first_exchange(self.bounds, r, wb, soff, [len(s) for s in send], seg[:-1] * wb, recv_bytes)
            sent = np.concatenate(send).view(np.float64).reshape(-1, k + 2)
            dp.assert_bits(sent, self.full[r], "the engine's records")
            self.step = 2
            return [self.segs[r][s].copy().view(np.uint8).reshape(-1) for s in range(W)]
        assert self.step == 3
        off = dp.output_offsets(self.bounds)
        for o in range(W):  # the padded blocks of the device: as many records as the owner received
            assert off[o + 1] - off[o] == sum(len(s) for s in self.segs[o]) == len(self.blocks[o])
        mine = self.blocks[r]
        for s in send:
            dp.assert_bits(s.view(np.float64).reshape(-1, k + 2), mine[mine[:, 0] >= 0], "the engine's block")
        dp.check_owner_block(mine, self.segs[r], *self.theta, self.lr, self.n, k, r == W - 1)
        self.step = 4
        return [b[b[:, 0] >= 0].copy().view(np.uint8).reshape(-1) for b in self.blocks]


@pytest.mark.parametrize("W,n_cols,B", [(2, 30, 1), (2, 30, 9), (8, 5, 3), (8, 70, 5), (8, 70, 53), (63, 40, 64),
                                        (63, 150, 64)])
def test_bookkeeping_against_the_numpy_engine(W, n_cols, B):
    k, lr = 3, 0.37
    rng = np.random.default_rng(100 * W + n_cols + B)
    log = gf._random_log(rng, 90, n_cols, 0.12, 1)
    theta = gf.perturbed_init(W, n_cols, k)
    ids = rng.permutation(90)[:B].astype(np.int32)
    # the ranges the harness cuts at are dist.owner_ranges, repeated starts included
    assert np.array_equal(np.clip(owner_ranges(n_cols, W), 0, n_cols), [n_cols * r // W for r in range(W)])
    after = []
    for r in sorted({0, W // 2, W - 1}):
        peers = HostPeers(log, k, lr, ids, W, r, theta)
        eng = _engine(log, k, lr, B, W, r, theta, peers)
        eng._step_rows(ids[slice(*shard_bounds(B, W, r))])
        assert peers.step == 4
        # the replica the engine is left with: the leader records, nothing else
        w0, w, V = (np.array(a, dtype=np.float64, copy=True) for a in theta)
        for b in peers.blocks:
            for rec in b[b[:, 0] >= 0]:
                c = int(rec[0])
                if c == n_cols:
                    w0[0] = rec[-1]
                else:
                    V[c], w[c] = rec[1:-1], rec[-1]
        for got, want in zip((eng.w0, eng.w, eng.V), (w0, w, V)):
            dp.assert_bits(got, want, f"replica of rank {r}")
        after.append((eng.w0.copy(), eng.w.copy(), eng.V.copy()))
    for other in after[1:]:  # every rank ends with the same bits
        for a, b in zip(after[0], other):
            dp.assert_bits(a, b, "replicas")


def test_rounding_candidates():
    """Both roundings of theta - lr * s pass, their neighbours do not; the two differ somewhere."""
    rng = np.random.default_rng(5)
    n, k, lr = 4, 2, 0.37
    seen_both = False
    for _ in range(200):
        V, w, w0 = rng.standard_normal((n, k)), rng.standard_normal(n), rng.standard_normal(1)
        segs = [np.concatenate([[[1.0]], rng.standard_normal((1, k + 1))], axis=1) for _ in range(3)]
        block = dp.owner_block(segs, w0, w, V, lr, n, k)
        dp.check_owner_block(block, segs, w0, w, V, lr, n, k, False)
        _, sums = dp.rank_order_sums(segs)
        theta = np.concatenate([V[1], [w[1]]])
        for f in range(k + 1):
            fused = dp.fused_update(theta[f], lr, sums[1][f])
            alt = block.copy()
            alt[0, 1 + f] = fused
            dp.check_owner_block(alt, segs, w0, w, V, lr, n, k, False)
            seen_both |= fused != block[0, 1 + f]
            for wrong in (np.nextafter(min(fused, block[0, 1 + f]), -np.inf), np.nextafter(max(fused, block[0, 1 + f]), np.inf)):
                alt[0, 1 + f] = wrong
                with pytest.raises(AssertionError):
                    dp.check_owner_block(alt, segs, w0, w, V, lr, n, k, False)
    assert seen_both


# --------------------------------------------------------------------------
# mutations of a recorded message
# --------------------------------------------------------------------------
@pytest.fixture(scope="module")
def recorded():
    """The messages of rank 3 of 8 for one iteration, peer 0's record of column 0 at 1e16 and peer 4's at
    -1e16 (rank order then changes the bits of the sum), and owner 0's block."""
    W, r, k, lr, B, n = 8, 3, 3, 0.37, 53, 70
    rng = np.random.default_rng(77)
    log = gf._random_log(rng, 90, n, 0.12, 1)
    theta = gf.perturbed_init(1, n, k)
    peers = HostPeers(log, k, lr, rng.permutation(90)[:B].astype(np.int32), W, r, theta)
    for s, v in ((0, 1e16), (4, -1e16)):
        assert peers.segs[0][s][0, 0] == 0.0
        peers.segs[0][s][0, 1:] = v
    block = dp.owner_block(peers.segs[0], *theta, lr, n, k)
    wb = (k + 2) * 8
    send, recv = dp.send_counts(peers.bounds, r), dp.recv_counts(peers.bounds, r)
    first = [(np.cumsum(send) - send) * wb, send * wb, (np.cumsum(recv) - recv) * wb, recv * wb]
    off = dp.output_offsets(peers.bounds)
    second = [np.full(W, off[r] * wb), np.full(W, (off[r + 1] - off[r]) * wb), off[:-1] * wb, np.diff(off) * wb]
    return types.SimpleNamespace(W=W, r=r, k=k, lr=lr, n=n, wb=wb, theta=theta, peers=peers, block=block,
                                 first=first, second=second)


def _check_block(m, block, segs=None):
    dp.check_owner_block(block, m.peers.segs[0] if segs is None else segs, *m.theta, m.lr, m.n, m.k, False)


def test_recorded_messages_pass(recorded):
    m = recorded
    dp.check_first_exchange(m.peers.bounds, m.r, m.wb, *m.first)
    dp.check_second_exchange(m.peers.bounds, m.r, m.wb, *m.second)
    _check_block(m, m.block)
    assert (m.first[1] > 0).all() and (m.block[:, 0] == -1).any()


def test_rejects_a_sum_in_reverse_rank_order(recorded):
    m = recorded
    segs = m.peers.segs[0]
    leader, _ = dp.rank_order_sums(segs)
    _, rev = dp.rank_order_sums(segs[::-1])
    block = m.block.copy()
    w0, w, V = m.theta
    for c, i in leader.items():
        block[i, 1:] = dp.plain_update(np.concatenate([V[c], [w[c]]]), m.lr, rev[c])
    assert (block[leader[0], 1:] != m.block[leader[0], 1:]).any()
    with pytest.raises(AssertionError, match="roundings"):
        _check_block(m, block)


def test_rejects_the_w0_record_sent_to_rank_0(recorded):
    m = recorded
    soff, sbytes, roff, rbytes = (a.copy() for a in m.first)
    sbytes[0] += m.wb
    sbytes[-1] -= m.wb
    soff[1:] += m.wb
    with pytest.raises(AssertionError, match="sbytes"):
        dp.check_first_exchange(m.peers.bounds, m.r, m.wb, soff, sbytes, roff, rbytes)


def test_rejects_a_range_start_off_by_one(recorded):
    m = recorded
    soff, sbytes, roff, rbytes = (a.copy() for a in m.first)
    soff[4] += m.wb
    sbytes[3] += m.wb
    sbytes[4] -= m.wb
    with pytest.raises(AssertionError):
        dp.check_first_exchange(m.peers.bounds, m.r, m.wb, soff, sbytes, roff, rbytes)
    soff = m.first[0].copy()
    soff[4] += m.wb  # the start alone
    with pytest.raises(AssertionError, match="soff"):
        dp.check_first_exchange(m.peers.bounds, m.r, m.wb, soff, *m.first[1:])


def test_rejects_a_leader_that_is_not_the_lowest_rank(recorded):
    m = recorded
    follower = np.flatnonzero(m.block[:, 0] == -1)[0]
    rows = np.concatenate(m.peers.segs[0])
    col = rows[follower, 0]
    lead = np.flatnonzero(m.block[:, 0] == col)[0]
    assert lead < follower
    block = m.block.copy()
    block[[lead, follower]] = block[[follower, lead]]
    with pytest.raises(AssertionError, match="column fields"):
        _check_block(m, block)


def test_rejects_roff_of_the_second_exchange_shifted(recorded):
    m = recorded
    soff, sbytes, roff, rbytes = (a.copy() for a in m.second)
    roff[1:] += m.wb
    with pytest.raises(AssertionError, match="roff"):
        dp.check_second_exchange(m.peers.bounds, m.r, m.wb, soff, sbytes, roff, rbytes)


def test_rejects_a_minus_one_record_carrying_a_column(recorded):
    m = recorded
    follower = np.flatnonzero(m.block[:, 0] == -1)[0]
    block = m.block.copy()
    block[follower, 0] = np.concatenate(m.peers.segs[0])[follower, 0]
    with pytest.raises(AssertionError, match="column fields"):
        _check_block(m, block)


# --------------------------------------------------------------------------
# the evaluator's tables: blocks, merge, and the mutations the comparison must reject
# --------------------------------------------------------------------------
def _random_tables(seed, lens, W, pad_extra=0, stride_extra=0):
    """A random table [vals | counted | order-dependent] of a log with groups of ``lens`` rows, cut for
    W ranks by dist.group_shard_bounds, and every rank's block with NaN padding."""
    from relevance_factorizationmachine_amd.dist import group_shard_bounds
    rng = np.random.default_rng(seed)
    n_seg = len(lens)
    seg = np.concatenate([[0], np.cumsum(lens)])
    lo = group_shard_bounds(seg, W).astype(np.int32)
    table = np.concatenate([rng.uniform(0.5, 3.0, n_seg), (rng.random(n_seg) < 0.7).astype(np.float64),
                            (rng.random(n_seg) < 0.2).astype(np.float64)])
    pad = max(int(np.diff(lo).max()), 1) + pad_extra
    stride = 3 * pad + stride_extra
    blocks = [dp.eval_block(table, lo[r], lo[r + 1], pad, stride, np.nan) for r in range(W)]
    return types.SimpleNamespace(table=table, lo=lo, pad=pad, stride=stride, blocks=blocks, n_seg=n_seg, W=W)


E_FEW = [3, 1, 64, 65, 2]


@pytest.mark.parametrize("W", [2, 8, 63])
@pytest.mark.parametrize("lens", [E_FEW, [2], [1, 129, 1], list(range(1, 41)), [2] * 300 + [129, 1, 65] + [2] * 90],
                         ids=["few", "one", "long-middle", "ramp", "many"])
@pytest.mark.parametrize("pad_extra,stride_extra", [(0, 0), (2, 5)])
def test_merge_of_the_blocks_is_the_table(W, lens, pad_extra, stride_extra):
    t = _random_tables(7 * W + len(lens), lens, W, pad_extra, stride_extra)
    assert t.lo[0] == 0 and t.lo[-1] == t.n_seg and (np.diff(t.lo) >= 0).all()
    if len(lens) < W:
        assert (np.diff(t.lo) == 0).sum() >= W - len(lens)  # fewer groups than ranks: ranks that own none
    for r in range(W):  # a block is the rank's rows and nothing else
        m = t.lo[r + 1] - t.lo[r]
        assert np.isnan(t.blocks[r]).sum() == t.stride - 3 * m
    dp.check_table(dp.merge_blocks(t.blocks, t.lo, t.pad, t.n_seg), t.table, "merge")
    for g in range(t.n_seg):
        r = dp.group_owner(t.lo, g)
        assert t.lo[r] <= g < t.lo[r + 1]


def test_e_few_bounds():
    """The two cuts test_gpu_dp_eval_ranks.py relies on."""
    from relevance_factorizationmachine_amd.dist import group_shard_bounds
    seg = np.concatenate([[0], np.cumsum(E_FEW)])
    assert group_shard_bounds(seg, 8).tolist() == [0, 3, 3, 3, 3, 4, 4, 4, 5]
    lo = group_shard_bounds(seg, 63)
    assert lo[:3].tolist() == [0, 1, 3] and lo[-1] == 5 and (np.diff(lo) == 0).sum() == 59


@pytest.fixture(scope="module")
def gathered():
    """E-few at 8 ranks (bounds 0 3 3 3 3 4 4 4 5: repeated starts in front of both later owners); the
    stride leaves room for a reader whose pad is one too large."""
    t = _random_tables(11, E_FEW, 8, 0, 4)
    assert t.lo.tolist() == [0, 3, 3, 3, 3, 4, 4, 4, 5] and t.pad == 3
    dp.check_table(dp.merge_blocks(t.blocks, t.lo, t.pad, t.n_seg), t.table, "merge")
    return t


def _rejected(t, merged):
    with pytest.raises(AssertionError):
        dp.check_table(merged, t.table, "a wrong merge")


def test_rejects_two_ranks_blocks_exchanged(gathered):
    t = gathered
    blocks = list(t.blocks)
    blocks[4], blocks[7] = blocks[7], blocks[4]  # both own one group
    _rejected(t, dp.merge_blocks(blocks, t.lo, t.pad, t.n_seg))


@pytest.mark.parametrize("off", [-1, 1])
def test_rejects_pad_off_by_one_on_the_reading_side(gathered, off):
    t = gathered
    _rejected(t, dp.merge_blocks(t.blocks, t.lo, t.pad + off, t.n_seg))


def test_rejects_a_block_read_at_u_where_pad_plus_u_is_meant(gathered):
    t = gathered
    _rejected(t, dp.merge_blocks(t.blocks, t.lo, t.pad, t.n_seg, parts=(0, 0, 2)))
    _rejected(t, dp.merge_blocks(t.blocks, t.lo, t.pad, t.n_seg, parts=(0, 1, 1)))


def test_rejects_a_padding_nan_read_in_place_of_a_value(gathered):
    t = gathered
    merged = dp.merge_blocks(t.blocks, t.lo, t.pad, t.n_seg, shift=1)  # rank 4's one group: u = 1 is padding
    assert np.isnan(merged[3])
    _rejected(t, merged)
    # ... and a NaN alone, in a table that is right everywhere else
    merged = dp.merge_blocks(t.blocks, t.lo, t.pad, t.n_seg)
    merged[t.n_seg + 3] = np.nan
    _rejected(t, merged)


def test_rejects_the_first_rank_whose_start_is_not_above_g_as_owner(gathered):
    """Groups 3 and 4 start at ranks 1 and 5 by that rule (ranks without groups), at ranks 4 and 7 by
    the right one: only repeated starts separate the two."""
    t = gathered

    def first_owner(lo, g):
        prev = [r for r in range(len(lo) - 1) if lo[r] <= g]
        return min(r for r in prev if lo[r] == max(lo[p] for p in prev))

    assert [first_owner(t.lo, g) for g in range(5)] == [0, 0, 0, 1, 5]
    assert [dp.group_owner(t.lo, g) for g in range(5)] == [0, 0, 0, 4, 7]
    _rejected(t, dp.merge_blocks(t.blocks, t.lo, t.pad, t.n_seg, owner=first_owner))
    # without repeated starts the two rules agree
    t2 = _random_tables(12, [2] * 16, 8)
    assert (np.diff(t2.lo) > 0).all()
    dp.check_table(dp.merge_blocks(t2.blocks, t2.lo, t2.pad, t2.n_seg, owner=first_owner), t2.table, "merge")


def test_stable_rule_table_ties_and_nan():
    """The later row first among equal scores; a tie between rows that differ, inside or across the
    first k ranks, or a NaN, flags the user; a user without a positive label does not count."""
    users = np.array([5, 5, 5, 2, 2, 9, 9, 9, 7, 7])
    frame = {"user": users, "label": np.array([1.0, 0, 0, 1, 0, 0, 0, 0, 0, 1]),
             "pscore": np.array([0.5, 0.5, 0.25, 1, 1, 1, 1, 1, 0.5, 0.5])}
    scores = np.array([0.3, 0.3, 0.1, 0.2, 0.9, 0.5, 0.5, 0.5, 0.4, np.nan])
    vals, counted, dep = dp.stable_rule_table(frame, scores, 1)
    # users ascending: 2 (distinct scores), 5 (rows 0 and 1 tie across rank 1, labels differ), 7 (NaN), 9 (no label)
    assert counted.tolist() == [True, True, True, False] and dep.tolist() == [False, True, True, False]
    assert vals[0] == 0.0 and vals[1] == 0.0 and vals[3] == 0.0  # user 5: the later row (label 0) ranks first
    vals, counted, dep = dp.stable_rule_table(frame, scores, 2)
    assert vals[1] == 1.0 / (0.5 * np.log2(2.0)) and vals[0] == 1.0 / np.log2(2.0)
