"""rfm_fm_fit_dp as one rank of 2, 8 and 63, the other ranks emulated in the same process
(dp_peers_common.EmulatedPeers): every message of the touched-rows and the dense exchange is checked
byte by byte and answered with what the peers would have sent, computed by the library's public entry
points on a second plan of the same log.  Needs an MI355X: ``pytest -m gpu``.

What is held exactly: the bounds a rank reports, the cuts of both all-to-all exchanges, the records a
rank sends (bit for bit where every sum has a fixed order, 1e-13 otherwise), every value an owner
emits (one of the two roundings of theta - lr * s, s the rank-ordered float64 sum), every row of the
replica after every iteration, the number of collectives.  What is held to a bound: every step against
the long-double SGD step of the global batch (gf.step_bound).  With RFM_DP_RANKS_MARGINS=<file> the
run's table of the largest error-over-bound ratios is written there (profiles/n24/dp_ranks_margins.txt
is one such run: a record, not a threshold)."""
import functools
import os

import numpy as np
import pytest

import dp_peers_common as dp
import forward_rows_common as fr
import grad_forms_common as gf

pytestmark = pytest.mark.gpu

LR = 0.37        # no power of two: lr * s rounds, so the fused and the plain update differ
N_ITERS = 3
K_BLOCKS = 64    # 32 lanes per row: every row of the log fits one round of a lane group
MARGINS = {}     # case -> largest step_excess ratio of the run


@pytest.fixture(scope="module")
def rt():
    from relevance_factorizationmachine_amd import runtime
    return runtime.Runtime.get()


@pytest.fixture(scope="module", autouse=True)
def margins_table():
    yield
    for case in _CASES.values():
        case.close()
    _CASES.clear()
    path = os.environ.get("RFM_DP_RANKS_MARGINS")
    if path and MARGINS:
        with open(path, "w") as f:
            f.write("largest |device step - long-double SGD step of the global batch| / gf.step_bound per case, "
                    f"over {N_ITERS} iterations (tests/test_gpu_dp_ranks.py)\n")
            for name, ratio in MARGINS.items():
                f.write(f"{name:<52} {ratio:.4f}\n")


# --------------------------------------------------------------------------
# logs and plans
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _log_a(n_rows=600):
    """600 rows x 2100 columns, about 6 entries per row and 2 dense columns: the columns cross the
    2048-column chunk of the compaction, and at 8 ranks the last owner range (from 1837) straddles it."""
    return gf._random_log(np.random.default_rng(2401), n_rows, 2100, 6 / 2100, 2)


@functools.lru_cache(maxsize=None)
def _log_b():
    """40 rows x 5 columns: fewer columns than ranks, the owner ranges at 8 ranks start at
    0, 0, 1, 1, 2, 3, 3, 4."""
    return gf._random_log(np.random.default_rng(2402), 40, 5, 0.5, 0)


PLANS = ("A-k8-hot-1", "A-k8-hot0", "A-k8-hot-2", "A-k65", "A-blocks", "B-k8")
_CASES = {}


def _case(rt, name):
    """The plan pair of a name, built once; every property the cases rely on is asserted here."""
    if name in _CASES:
        return _CASES[name]
    if name == "B-k8":
        case = dp.PeerCase(rt, _log_b(), 8, 40, 0)
        assert dp.owner_ranges(5, 8).tolist() == [0, 0, 1, 1, 2, 3, 3, 4]
    elif name == "A-blocks":
        # as many rows as the many-rows forward needs at this factor count, no more
        n_rows = max(600, fr.many_rows_minimum(rt, K_BLOCKS, True))
        case = dp.PeerCase(rt, _log_a(n_rows), K_BLOCKS, n_rows, 0)
        assert case.dev.plan.layout()["row_blocks"] == 1, case.dev.plan.layout()
    else:
        k, hot = {"A-k8-hot-1": (8, -1), "A-k8-hot0": (8, 0), "A-k8-hot-2": (8, -2), "A-k65": (65, 0)}[name]
        case = dp.PeerCase(rt, _log_a(), k, 64, hot)
        n_hot = case.dev.plan.info()["hot_columns"]
        assert case.dev.plan.layout()["row_blocks"] == 0
        assert (n_hot > 0) == (hot in (0, -2) and k == 8), (name, n_hot)
        if k == 8:
            # fixed-order hot sums, as the plan's forms report them: a small batch's train-loss rows
            # ride in the next step's forward unless the plan sums its hot columns in a fixed order
            ride = fr.train_forms(rt, case.dev.plan, 64, 8, 0, None, 0, True, False)["ride"]
            assert ride == (0 if hot == -2 else 1), (name, ride)
        assert case.dev.plan.layout()["lanes_per_row"] == gf.CLASS_OF[k][0]
    if name.startswith("A"):
        assert case.n == 2100 and dp.owner_ranges(2100, 8)[7] == 1837 < 2048 < 2100
    _CASES[name] = case
    return case


@functools.lru_cache(maxsize=None)
def _theta(n, k):
    return gf.perturbed_init(24 + k, n, k)


def _ids(case, B, n_iters, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.permutation(case.dev.n_rows)[:B] for _ in range(n_iters)]).astype(np.int32)


def _clean_call(rt, case, W, B, r, mode, seed=0, inject=None, name=None):
    """One call with every check; returns the peers."""
    params = dp.GuardedParams(rt, *_theta(case.n, case.k))
    peers = dp.EmulatedPeers(case, W, r, _ids(case, B, N_ITERS, 1000 * W + B + seed), params, LR, mode, inject=inject)
    rc = peers.run()
    assert rc == 0, peers.message  # (bounds_check_kernel raised nothing)
    peers.check_counts()
    peers.check_replica()
    if inject is None:
        ratio = peers.oracle_excess()
        if name:
            MARGINS[name] = ratio
        print(f"{name}: largest step excess {ratio:.4f}")
        assert ratio <= 1.0, ratio
    return peers


# --------------------------------------------------------------------------
# the worlds
# --------------------------------------------------------------------------
WORLDS_A = [(8, 5, (0, 3, 5, 7)), (8, 203, (0, 3, 7)), (63, 64, (0, 31, 62)), (2, 1, (0, 1))]
CASES = [(plan, W, B, r, mode) for plan in PLANS[:-1] for W, B, ranks in WORLDS_A for r in ranks
         for mode in (("rows", "dense") if W == 8 else ("rows",))]
CASES += [("B-k8", 8, 3, r, mode) for r in (0, 3, 7) for mode in ("rows", "dense")]


@pytest.mark.parametrize("plan,W,B,r,mode", CASES, ids=[f"{p}-W{W}-B{B}-r{r}-{m}" for p, W, B, r, m in CASES])
def test_one_rank_among_emulated_peers(rt, plan, W, B, r, mode):
    case = _case(rt, plan)
    lo, hi = dp.shard_bounds(B, W, r)
    if (W, B) == (8, 5):
        assert (hi == lo) == (r >= 5)  # ranks 5-7 hold no row
    if (W, B) == (63, 64):
        assert hi - lo == (2 if r == 0 else 1)
    _clean_call(rt, case, W, B, r, mode, name=f"{plan} W={W} B={B} rank={r} {mode}")


@pytest.mark.parametrize("plan", ["A-k8-hot-1", "A-k8-hot0", "A-k65"])
def test_rank_order_of_the_owner_sum(rt, plan):
    """Peer 1 sends 1e16 and peer 5 -1e16 for dense column 0, which rank 3's shard touches too: the bits
    of the sum depend on the order, and only the rank order passes."""
    case = _case(rt, plan)
    peers = _clean_call(rt, case, 8, 203, 3, "rows", seed=7, inject=(0, 1, 5))
    s = dp.rank_order_sums(peers.segs[0])[1][0]
    rev = dp.rank_order_sums(peers.segs[0][::-1])[1][0]
    assert (s != rev).any()


# --------------------------------------------------------------------------
# the loss sums of an idle rank
# --------------------------------------------------------------------------
def test_loss_sums_of_an_idle_rank(rt):
    """Rank 6 of 8 at a global batch of 5 and 5 validation rows holds neither: over 130 iterations (one
    more than a run of 128) its sums arrive as exact zeros, and the outputs are the answer scaled."""
    from relevance_factorizationmachine_amd.runtime import DeviceCSR
    case = _case(rt, "A-k8-hot0")
    n_iters, W, B, r = 130, 8, 5, 6
    assert dp.shard_bounds(B, W, r) == (5, 5) and dp.shard_bounds(5, W, r) == (5, 5)
    vlog = gf._random_log(np.random.default_rng(9), 5, case.n, 6 / 2100, 2)
    val = (DeviceCSR(rt, vlog["features"]), rt.upload(vlog["labels"], dtype=np.float64),
           rt.upload(vlog["pscores"], dtype=np.float64))
    S = np.random.default_rng(10).standard_normal(2 * n_iters)
    params = dp.GuardedParams(rt, *_theta(case.n, case.k))
    peers = dp.EmulatedPeers(case, W, r, _ids(case, B, n_iters, 11), params, LR, "rows", loss_answer=S,
                             aux_bounds=False)
    assert peers.run(val=val, want_losses=True) == 0, peers.message
    peers.check_counts(losses=True)
    peers.check_replica()
    seen = peers.loss_seen
    assert seen.shape == (2 * n_iters,) and not seen.any() and not np.signbit(seen).any()
    dp.assert_bits(peers.out_train.cpu().numpy(), -S[:n_iters] / 5.0, "train losses")
    dp.assert_bits(peers.out_val.cpu().numpy(), -S[n_iters:] / 5.0, "validation losses")


# --------------------------------------------------------------------------
# error returns (none of them a fault: every transfer stays within what exists)
# --------------------------------------------------------------------------
def _failing_call(rt, case, W, B, r, mode, **kw):
    params = dp.GuardedParams(rt, *_theta(case.n, case.k))
    peers = dp.EmulatedPeers(case, W, r, _ids(case, B, N_ITERS, 5), params, LR, mode, **kw)
    rc = peers.run()
    params.host()  # (the guard rows)
    return peers, rc


@pytest.mark.parametrize("name,mode,index", [("all_gather", "rows", 0), ("all_to_all", "rows", 0),
                                             ("all_to_all", "rows", 3), ("all_reduce_sum", "dense", 1)])
def test_a_failing_collective_is_named(rt, name, mode, index):
    from relevance_factorizationmachine_amd import _lib
    case = _case(rt, "A-k8-hot0")
    peers, rc = _failing_call(rt, case, 8, 203, 3, mode, fail=(name, index))
    assert rc == _lib.RFM_ERR_INTERNAL and f"transport {name} failed" in peers.message, (rc, peers.message)
    assert peers.calls[name] == index + 1
    _clean_call(rt, case, 8, 203, 3, mode, seed=1)  # the plan stays usable


def test_corrupt_gathered_bounds_are_refused_before_the_loop(rt):
    from relevance_factorizationmachine_amd import _lib
    case = _case(rt, "A-k8-hot0")

    def tamper(table):  # peer 5's list, iteration 1: range 3 would start behind range 4
        table[5, 1, 3] = table[5, 1, 4] + 1

    peers, rc = _failing_call(rt, case, 8, 203, 3, "rows", tamper=tamper)
    assert rc == _lib.RFM_ERR_BAD_ARG and "corrupt bounds" in peers.message, (rc, peers.message)
    assert peers.calls == {"all_gather": 1, "all_to_all": 0, "all_reduce_sum": 0}
    for got, want in zip(peers.params.host(), peers.theta0):
        dp.assert_bits(got, want, "the replica of a refused call")
    _clean_call(rt, case, 8, 203, 3, "rows", seed=2)


def test_a_list_longer_than_planned_raises_the_flag(rt):
    """The rank's own row of the gathered table says one record fewer than its steps produce: every
    transfer moves fewer records than exist (the emulation asserts it), and the call ends with the error
    of bounds_check_kernel's flag, naming the first iteration."""
    from relevance_factorizationmachine_amd import _lib
    case = _case(rt, "A-k8-hot0")
    W, r = 8, 3

    def tamper(table):
        assert (table[r, :, W] > table[r, :, W - 1]).all()  # (stays monotone)
        table[r, :, W] -= 1

    peers, rc = _failing_call(rt, case, W, 203, r, "rows", tamper=tamper)
    assert rc == _lib.RFM_ERR_INTERNAL and "iteration 0" in peers.message and "do not match" in peers.message, (
        rc, peers.message)
    assert peers.calls == {"all_gather": 1, "all_to_all": 2 * N_ITERS, "all_reduce_sum": 0}
    _clean_call(rt, case, W, 203, r, "rows", seed=3)


# --------------------------------------------------------------------------
# stamps
# --------------------------------------------------------------------------
def test_stamps_do_not_leak_between_calls(rt):
    """Rows, dense, rows on one plan, back to back, another rank each time (a rows call reserves stamps
    twice): a record of an earlier call or iteration would break the bounds or the record comparison."""
    case = _case(rt, "A-k8-hot-2")
    for seed, (r, mode, B) in enumerate([(0, "rows", 203), (3, "dense", 203), (7, "rows", 5), (3, "rows", 203)]):
        _clean_call(rt, case, 8, B, r, mode, seed=40 + seed)
