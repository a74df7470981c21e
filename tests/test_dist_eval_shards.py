"""How ``dist.fit_data_parallel`` cuts a ValEvaluator's log among the ranks (no GPU):
``group_shard_bounds`` over user groups, and a rank's shard (``ValFrame.take_groups``) redoing its
tie-order dependent users exactly as the whole frame would."""
import numpy as np
import pytest

from relevance_factorizationmachine_amd.dist import group_shard_bounds
from relevance_factorizationmachine_amd.evaluate import ValFrame, group_by_user


def _check_bounds(seg_ptr, world):
    seg = np.asarray(seg_ptr, dtype=np.int64)
    n_groups, total = seg.shape[0] - 1, int(seg[-1])
    lo = group_shard_bounds(seg, world)
    assert lo.shape == (world + 1,)
    assert lo[0] == 0 and lo[-1] == n_groups  # covers every group
    assert np.all(np.diff(lo) >= 0)  # monotone, hence contiguous ranges that do not overlap
    ideal = total / world
    for r in range(world):
        a, b = int(lo[r]), int(lo[r + 1])
        if a == b:
            continue
        # without its last group a rank stays within the ideal row share
        assert seg[b - 1] - seg[a] <= ideal, (world, r, a, b)
    return lo


@pytest.mark.parametrize("world", [1, 2, 3, 4, 7, 16])
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_group_shard_bounds_random_groups(world, seed):
    rng = np.random.default_rng(seed)
    lens = rng.integers(1, 40, size=int(rng.integers(1, 300)))
    lens[rng.integers(0, lens.shape[0])] = 500  # one long group
    _check_bounds(np.concatenate([[0], np.cumsum(lens)]), world)


def test_group_shard_bounds_more_ranks_than_groups():
    seg = np.array([0, 5, 9])
    lo = _check_bounds(seg, 5)
    assert np.count_nonzero(np.diff(lo)) == 2  # three ranks hold no group
    lo = _check_bounds(np.array([0, 100]), 3)
    assert list(lo) == [0, 1, 1, 1]
    assert list(_check_bounds(np.array([0]), 3)) == [0, 0, 0, 0]  # an empty log


def test_group_shard_bounds_balances_rows():
    seg = np.arange(0, 1001, 10)  # 100 groups of 10 rows
    lo = _check_bounds(seg, 4)
    assert list(lo) == [0, 25, 50, 75, 100]
    with pytest.raises(ValueError):
        group_shard_bounds(seg, 0)


@pytest.mark.parametrize("world", [2, 3])
def test_shards_redo_tied_users_as_the_whole_frame(world):
    """Every rank recomputes its own flagged users from its shard's scores; put together they
    are the whole frame's ``host_user_values`` (the same per-user arrays, the same argsort)."""
    rng = np.random.default_rng(3)
    users = rng.integers(0, 60, size=900)
    labels = rng.integers(0, 2, size=900).astype(np.float64)
    pscores = rng.uniform(0.1, 1.0, size=900)
    scores = np.round(rng.uniform(size=900), 1)  # many ties
    fr = ValFrame(users, labels, pscores, k=5)
    want = fr.host_user_values(scores, np.arange(fr.n_segments))
    order, _ = group_by_user(users)
    lo = group_shard_bounds(fr.h_seg_ptr, world)
    got = np.empty(fr.n_segments)
    for r in range(world):
        part = fr.take_groups(int(lo[r]), int(lo[r + 1]))
        r0 = int(fr.h_seg_ptr[lo[r]])
        shard_scores = scores[order[r0: r0 + part.n_rows]]  # the shard's rows, grouped order
        got[lo[r]: lo[r + 1]] = part.host_user_values(shard_scores, np.arange(part.n_segments))
    np.testing.assert_array_equal(got, want)
