"""rfm_fm_fit_dp_eval as one rank of 2, 8 and 63, the other ranks emulated in the same process
(dp_peers_common.EmulatedPeers with an EvalArgs): on top of every check of the step
(test_gpu_dp_ranks.py) the evaluator's one all-gather is checked byte by byte and answered with what
the peers would have sent, and everything the call leaves is compared with the whole evaluation log
scored by rfm_fm_plan_forward and ranked by rfm_val_dcg on a second plan.  Needs an MI355X:
``pytest -m gpu``.

Bit for bit, in every case: the shard's scores in d_scores against the whole log's; the rank's message
(its groups' rows of the reference table at [u | pad + u | 2 pad + u], +0.0 in every other double);
d_user_scratch against that message; d_full_out against the reference table; d_dcg_out against
rfm_val_dcg's two results (NaN against NaN where no user counts); every double around those outputs
(columns behind the shard's rows, slots outside the call, a slot in front and one behind) still NaN.
The peers' padding is NaN, so a merge or a mean that reads it cannot pass.
At 1e-12 relative (tests/test_gpu_eval.py TOL: float64 on both sides, the reference's term order per
user, another fixed order over users): the reference table's values and mean against the tie rule
restated in NumPy (dp.stable_rule_table); its counted and order-dependent flags are equal exactly.

Every plan of test_gpu_dp_ranks.py (and A-k130, a plan with slices) meets every world, rank and log of
GRID; a case takes a few tenths of a second."""
import functools

import numpy as np
import pytest

import dp_peers_common as dp
import grad_forms_common as gf
import test_gpu_dp_ranks as dr
from relevance_factorizationmachine_amd.dist import group_shard_bounds
from test_gpu_dp_ranks import LR, N_ITERS

pytestmark = pytest.mark.gpu

_WHOLE = {}  # (plan, log) -> dp.EvalCase


@pytest.fixture(scope="module")
def rt():
    from relevance_factorizationmachine_amd import runtime
    return runtime.Runtime.get()


@pytest.fixture(scope="module", autouse=True)
def close_plans():
    yield
    _WHOLE.clear()
    for case in dr._CASES.values():
        case.close()
    dr._CASES.clear()


# --------------------------------------------------------------------------
# evaluation logs
# --------------------------------------------------------------------------
CYCLE = (1, 2, 3, 63, 64, 65, 129)   # around one and two rounds of a wavefront, shorter and longer than k
ZERO_USERS = (0, 550, 1099)          # groups without a positive label
COPY_USERS = tuple(range(200, 214)) + (82, 107, 132, 157, 257, 282)  # groups with a row copied, 2 to 129 rows
FEW = (3, 1, 64, 65, 2)


def _frame_log(rng, lens, n_cols, positive):
    """gf._random_log of sum(lens) rows in a shuffled frame order; group g is user 3 g + 1."""
    n_rows = int(np.sum(lens))
    raw = gf._random_log(rng, n_rows, n_cols, *((6 / 2100, 2) if n_cols == 2100 else (0.5, 0)))
    users = np.repeat(3 * np.arange(len(lens)) + 1, lens)[rng.permutation(n_rows)]
    labels = raw["labels"] if positive is None else rng.random(n_rows) < positive
    return raw["features"], users, labels.astype(np.float64), raw["pscores"]


@functools.lru_cache(maxsize=None)
def _e_many(n_cols):
    """1 100 users, 4 078 rows: 42 users cycle through CYCLE, every 25th from user 7 on, the rest have
    2 rows; labels positive at 8 %, none for ZERO_USERS; in each of COPY_USERS one row is the exact
    copy of another with the other label (they tie at any parameters)."""
    rng = np.random.default_rng(2501)
    lens = np.full(1100, 2)
    lens[7 + 25 * np.arange(42)] = np.resize(CYCLE, 42)
    X, users, labels, p = _frame_log(rng, lens, n_cols, 0.08)
    assert X.shape[0] == 4078 < 4096  # (under the default RFM_SLICED_MIN_ROWS)
    for g in ZERO_USERS:
        labels[users == 3 * g + 1] = 0.0
    src = np.arange(X.shape[0])
    for g in COPY_USERS:
        rows = np.flatnonzero(users == 3 * g + 1)
        assert len(rows) >= 2 and g not in ZERO_USERS
        src[rows[-1]] = rows[0]
        labels[rows[0]], labels[rows[-1]] = 1.0, 0.0
    assert len(COPY_USERS) == 20
    log = dp.EvalLog(X[src], users, labels, p)
    assert log.n_seg == 1100 and np.array_equal(np.diff(log.seg), lens)
    return log


@functools.lru_cache(maxsize=None)
def _e_few(n_cols, zero=False):
    rng = np.random.default_rng(2502)
    X, users, labels, p = _frame_log(rng, FEW, n_cols, None)
    if zero:
        labels[:] = 0.0
    log = dp.EvalLog(X, users, labels, p)
    assert np.array_equal(np.diff(log.seg), FEW)
    assert group_shard_bounds(log.seg, 8).tolist() == [0, 3, 3, 3, 3, 4, 4, 4, 5]  # ranks 1-3, 5, 6 own nothing
    lo63 = group_shard_bounds(log.seg, 63)
    assert lo63[:3].tolist() == [0, 1, 3] and (np.diff(lo63) == 0).sum() == 59
    assert [r for r in range(63) if lo63[r + 1] > lo63[r]] == [0, 1, 31, 62]
    return log


def _log(name, n_cols):
    if name == "many":
        return _e_many(n_cols)
    if name == "many-ones":
        return _e_many(n_cols).with_ones()
    return _e_few(n_cols, zero=(name == "few-zero"))


def _case(rt, name):
    """The plan pairs of test_gpu_dp_ranks.py, and A-k130: log A at 130 factors, a plan with slices."""
    if name != "A-k130":
        return dr._case(rt, name)
    if name not in dr._CASES:
        case = dp.PeerCase(rt, dr._log_a(), 130, 64, 0)
        assert case.dev.plan.sliced()["slices"] >= 1 and case.aux.plan.sliced() == case.dev.plan.sliced()
        assert case.dev.plan.layout()["row_blocks"] == 0 and case.fixed
        dr._CASES[name] = case
    return dr._CASES[name]


def _whole(rt, plan, log):
    if (plan, log) not in _WHOLE:
        case = _case(rt, plan)
        _WHOLE[(plan, log)] = dp.EvalCase(case, _log(log, case.n))
    return _WHOLE[(plan, log)]


def _peers(rt, plan, W, B, r, mode, log, k, n_iters=N_ITERS, seed=0, ev_kw=None, **peer_kw):
    case = _case(rt, plan)
    params = dp.GuardedParams(rt, *dr._theta(case.n, case.k))
    peers = dp.EmulatedPeers(case, W, r, dr._ids(case, B, n_iters, 1000 * W + B + seed), params, LR, mode, **peer_kw)
    return peers, dp.EvalArgs(rt, _whole(rt, plan, log), W, r, k, n_iters, **(ev_kw or {}))


def _clean_call(rt, plan, W, B, r, mode, log, k, seed=0, **ev_kw):
    """One call with every check of the step and of the evaluator; returns the peers and the arguments."""
    peers, ea = _peers(rt, plan, W, B, r, mode, log, k, seed=seed, ev_kw=ev_kw)
    rc = peers.run(ev=ea)
    assert rc == 0, peers.message
    peers.check_counts(evaluator=True)
    peers.check_replica()
    ratio = peers.oracle_excess()
    assert ratio <= 1.0, ratio
    peers.check_evaluator()
    if log.startswith("many"):
        assert all(out[1] > 0 for _, _, out in peers.ref), "the copied rows make no user order-dependent"
    return peers, ea


# --------------------------------------------------------------------------
# the worlds
# --------------------------------------------------------------------------
# (W, B, log, k, ranks): the first rank, the last rank that owns groups, a rank that owns none between
# two owners (rank 2 of 8 and rank 30 of 63 on E-few, rank 8 of 63 on E-many), the last rank; rank 6 of
# 63 on E-many holds one group of two rows
GRID = [(2, 1, "many", 5, (0, 1)), (8, 5, "few", 5, (0, 2, 7)), (8, 5, "few", 9, (0, 2, 7)),
        (8, 203, "many", 5, (0, 3, 7)), (63, 64, "many", 5, (0, 6, 8, 62)), (63, 64, "few", 9, (0, 30, 62))]
A_PLANS = ("A-k8-hot0", "A-k8-hot-1", "A-k65", "A-blocks", "A-k130")
# log B has 40 rows: the worlds whose global batch fits it
CASES = [(plan, W, B, r, mode, log, k) for plan in A_PLANS + ("B-k8",) for W, B, log, k, ranks in GRID
         if plan != "B-k8" or B <= 40 for r in ranks for mode in (("rows", "dense") if W == 8 else ("rows",))]
CASES += [("A-k8-hot0", 8, 5, r, "rows", "few-zero", 5) for r in (0, 2)]  # nobody has a positive label
CASES += [("B-k8", 8, 5, 7, "rows", "many", 5)]


def _owned(log, W, r):
    lo = group_shard_bounds(log.seg, W)
    return int(lo[r]), int(lo[r + 1]), lo


@pytest.mark.parametrize("plan,W,B,r,mode,log,k", CASES,
                         ids=[f"{p}-W{W}-B{B}-r{r}-{m}-{lg}-k{k}" for p, W, B, r, m, lg, k in CASES])
def test_one_rank_among_emulated_peers(rt, plan, W, B, r, mode, log, k):
    elog = _log(log, _case(rt, plan).n)
    g0, g1, lo = _owned(elog, W, r)
    owners = [s for s in range(W) if lo[s + 1] > lo[s]]
    if log.startswith("few"):
        assert k in (5, 9) and (np.diff(elog.seg) < 9).sum() == 3  # k = 9: longer than three of the groups
        if (W, r) in ((8, 2), (63, 30)):
            assert g1 == g0 and min(owners) < r < max(owners)
        if (W, r) in ((8, 7), (63, 62)):
            assert g1 > g0 and r == max(owners) == W - 1
    if log == "many" and W == 63:
        assert len(owners) == 57
        if r == 8:
            assert g1 == g0 and 7 in owners and 9 in owners
        if r == 6:
            assert g1 - g0 == 1 and elog.seg[g1] - elog.seg[g0] == 2
    if log == "many" and W == 8:
        on_real = [g0 <= g < g1 for g in ZERO_USERS]
        assert any(on_real) and not all(on_real)  # a user without a positive label here, another at a peer
    peers, ea = _clean_call(rt, plan, W, B, r, mode, log, k)
    if log == "few-zero":
        assert all(np.isnan(out[0]) and out[1] == 0 for _, _, out in peers.ref)
        assert np.isnan(ea.dcg.host()[1: 1 + N_ITERS, 0]).all()


# --------------------------------------------------------------------------
# what the ABI allows and the driver never passes
# --------------------------------------------------------------------------
def _natural_pad(rt, W):
    return int(np.diff(group_shard_bounds(_e_many(2100).seg, W)).max())


@pytest.mark.parametrize("variant", ["strides", "scores_stride", "slot_first", "rows", "null_pscores"])
def test_argument_variants(rt, variant):
    W, B, r, log, kw = 8, 203, 3, "many", {}
    pad = _natural_pad(rt, W)
    if variant == "strides":
        kw = dict(pad=pad + 2, user_stride=3 * (pad + 2) + 5)
    elif variant == "scores_stride":
        kw = dict(scores_extra=3)
    elif variant == "slot_first":
        kw = dict(slot_first=2)
    elif variant == "rows":  # the shard's CSR in a shuffled order, d_rows: grouped position -> CSR row
        kw = dict(permute=17)
    else:  # d_ev_pscores = NULL against a reference with all-ones propensities
        kw, log = dict(ones=True), "many-ones"
    peers, ea = _clean_call(rt, "A-k8-hot0", W, B, r, "rows", log, 5, seed=3, **kw)
    if variant == "strides":
        assert ea.pad == pad + 2 > ea.n_local and ea.user_stride == 3 * ea.pad + 5
    if variant == "scores_stride":
        assert ea.scores_stride == ea.n_ev + 3
    if variant == "rows":
        assert not np.array_equal(ea.h_rows, np.arange(ea.n_ev)) and ea.rows is not None
    if variant == "null_pscores":
        assert ea.pscores is None


# --------------------------------------------------------------------------
# a run longer than the loss run of 128 iterations
# --------------------------------------------------------------------------
def test_130_iterations_of_an_idle_rank(rt):
    """Rank 6 of 8 at a global batch of 5, 5 validation rows and E-few holds no row of any of them:
    130 tables and 130 means as in every other case, and its loss sums still arrive as exact zeros."""
    from relevance_factorizationmachine_amd.runtime import DeviceCSR
    case = _case(rt, "A-k8-hot0")
    n_iters, W, B, r = 130, 8, 5, 6
    assert dp.shard_bounds(B, W, r) == (5, 5) and _owned(_e_few(case.n), W, r)[:2] == (4, 4)
    vlog = gf._random_log(np.random.default_rng(9), 5, case.n, 6 / 2100, 2)
    val = (DeviceCSR(rt, vlog["features"]), rt.upload(vlog["labels"], dtype=np.float64),
           rt.upload(vlog["pscores"], dtype=np.float64))
    S = np.random.default_rng(10).standard_normal(2 * n_iters)
    peers, ea = _peers(rt, "A-k8-hot0", W, B, r, "rows", "few", 5, n_iters=n_iters, loss_answer=S, aux_bounds=False)
    assert ea.n_ev == 0 and ea.n_local == 0
    assert peers.run(val=val, want_losses=True, ev=ea) == 0, peers.message
    peers.check_counts(losses=True, evaluator=True)
    peers.check_replica()
    peers.check_evaluator()
    assert len(peers.ref) == n_iters
    seen = peers.loss_seen
    assert seen.shape == (2 * n_iters,) and not seen.any() and not np.signbit(seen).any()
    dp.assert_bits(peers.out_train.cpu().numpy(), -S[:n_iters] / 5.0, "train losses")
    dp.assert_bits(peers.out_val.cpu().numpy(), -S[n_iters:] / 5.0, "validation losses")


# --------------------------------------------------------------------------
# a tiny shard in the whole log's form
# --------------------------------------------------------------------------
@pytest.mark.parametrize("r", [6, 13])
def test_a_tiny_shard_scores_in_the_whole_logs_form(rt, monkeypatch, r):
    """63 ranks on E-many with a plan that has slices: rank 6 holds one group of 2 rows, rank 13
    nine groups of 18.  With RFM_SLICED_MIN_ROWS between the two row counts the whole log takes the
    sliced forward and the shard alone would not; with the default both take the plain one.  Either
    way the shard's scores are the whole log's, bit for bit (check_evaluator)."""
    case = _case(rt, "A-k130")
    elog = _e_many(case.n)
    g0, g1, _ = _owned(elog, 63, r)
    n_ev, n_total = int(elog.seg[g1] - elog.seg[g0]), elog.n_rows
    assert 1 <= g1 - g0 <= 18 and n_ev == {6: 2, 13: 18}[r]
    monkeypatch.setenv("RFM_SLICED_MIN_ROWS", "4000")
    for plan in (case.dev.plan, case.aux.plan):
        assert plan.sliced_geometry(n_total)["sliced"] == 1 and plan.sliced_geometry(n_ev)["sliced"] == 0
        assert plan.sliced_geometry(n_ev, n_total)["sliced"] == 1
    _clean_call(rt, "A-k130", 63, 64, r, "rows", "many", 5, seed=1)
    monkeypatch.delenv("RFM_SLICED_MIN_ROWS")
    for plan in (case.dev.plan, case.aux.plan):
        assert plan.sliced_geometry(n_total)["sliced"] == 0 and plan.sliced_geometry(n_ev, n_total)["sliced"] == 0
    _clean_call(rt, "A-k130", 63, 64, r, "rows", "many", 5, seed=2)


# --------------------------------------------------------------------------
# error returns (none of them a fault: every transfer stays within what exists)
# --------------------------------------------------------------------------
def test_a_failing_evaluator_all_gather_is_named(rt):
    from relevance_factorizationmachine_amd import _lib
    peers, ea = _peers(rt, "A-k8-hot0", 8, 203, 3, "rows", "many", 5, seed=5, fail=("all_gather", 1))
    rc = peers.run(ev=ea)
    assert rc == _lib.RFM_ERR_INTERNAL and "transport all_gather failed" in peers.message, (rc, peers.message)
    assert peers.calls == {"all_gather": 2, "all_to_all": 2 * N_ITERS, "all_reduce_sum": 0}
    peers.params.host()  # (the guard rows)
    assert np.isnan(ea.full.host()).all() and np.isnan(ea.dcg.host()).all()
    _clean_call(rt, "A-k8-hot0", 8, 203, 3, "rows", "many", 5, seed=6)  # the plan stays usable


def _lo0(ea):
    ea.group_lo[0] = 1


def _decreasing(ea):
    ea.group_lo[6] = ea.group_lo[5] - 1


def _over_pad(ea):
    assert ea.n_local < ea.pad
    ea.pad = ea.n_local  # (user_stride stays 3 times the old one)


def _n_local(ea):
    ea.n_local -= 1


def _user_stride(ea):
    ea.user_stride = 3 * ea.pad - 1


def _k0(ea):
    ea.k = 0


@pytest.mark.parametrize("edit,cause", [(_lo0, "group bounds do not cover"), (_decreasing, "group bounds of rank 5"),
                                        (_over_pad, "group bounds of rank"), (_n_local, "bounds say"),
                                        (_user_stride, "bad evaluation shape"), (_k0, "k=0")],
                         ids=["first-bound-not-0", "decreasing-pair", "more-groups-than-pad", "n_local_segments",
                              "user_stride", "k-0"])
def test_bad_evaluation_arguments_are_refused_before_anything_moves(rt, edit, cause):
    from relevance_factorizationmachine_amd import _lib
    peers, ea = _peers(rt, "A-k8-hot0", 8, 203, 3, "rows", "many", 5, seed=7)
    edit(ea)
    rc = peers.run(ev=ea)
    assert rc == _lib.RFM_ERR_BAD_ARG and cause in peers.message, (rc, peers.message)
    assert peers.calls == {"all_gather": 0, "all_to_all": 0, "all_reduce_sum": 0}
    for got, want in zip(peers.params.host(), peers.theta0):
        dp.assert_bits(got, want, "the replica of a refused call")
    ea.outputs_untouched()
