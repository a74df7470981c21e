"""rfm_diverse_select on the device through the raw ABI: every case byte for byte
against the float64 statement of diverse_common.py in all four outputs, and against the long-double
oracle -- the same item at every step, the value within its derived tolerance -- with sentinels
behind every output.  The shapes are the edges of the lane loop (factors), of the thread stride
(depth) and of the grid (lists), not a workload; test_diverse_host.py asserts that every step of
every random case list is separated and that the checkers used here refuse six mutations.  Needs
an MI355X: ``pytest -m gpu``.

On the code before this feature every test here fails: the entries do not exist."""
import numpy as np
import pytest

import diverse_common as dc
from fold_common import _n_cu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rfm():
    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import features, recommend, runtime
    return pkg, features, recommend, runtime.Runtime.get()


def _check(rfm, c, penalty, lam, k, what, oracle=True, **strides):
    got = dc.select(rfm, c.items, c.scores, c.R, c.kf, penalty, lam, k, **strides)
    want = dc.select_statement(c.items, c.scores, c.R, c.kf, penalty, lam, k)
    dc.assert_same_bits(got, want, what)
    if oracle:
        dc.assert_against_oracle(got, dc.select_oracle(c.items, c.scores, c.R, c.kf, penalty, lam, k), c.scores, what)
    return got


@pytest.mark.parametrize("stride", ["k", "kpad"])
@pytest.mark.parametrize("kf", dc.GPU_FACTORS)
def test_factor_counts(rfm, kf, stride):
    c = dc.case(dc.GPU_LISTS, 65, kf)
    assert dc.geometry(c.n_lists, 65, kf)["factor_trips"] == -(-kf // 64)
    ld_R = kf if stride == "k" else dc.pad4(kf)
    _check(rfm, c, None, 0.3, 9, f"factors={kf} ld_R={ld_R}", ld_R=ld_R)
    _check(rfm, c, c.penalty, 0.7, 9, f"factors={kf} ld_R={ld_R} penalty", ld_R=ld_R)


@pytest.mark.parametrize("kf", dc.GPU_DEPTH_FACTORS)
@pytest.mark.parametrize("depth", dc.GPU_DEPTHS)
def test_depths(rfm, depth, kf):
    c = dc.case(dc.GPU_LISTS, depth, kf)
    assert dc.geometry(c.n_lists, depth, kf)["candidates_per_thread"] == -(-depth // dc.BLOCK)
    got = _check(rfm, c, None, 0.7, 9, f"depth={depth} factors={kf}")
    assert ((got[3] >= 0).sum(axis=1) == min(9, depth)).all()  # (depth 1, 2: fewer candidates than picks, pads)
    _check(rfm, c, c.penalty, 0.3, 9, f"depth={depth} factors={kf} penalty")


@pytest.mark.parametrize("k", dc.GPU_K)
def test_pick_counts(rfm, k):
    c = dc.case(dc.GPU_LISTS, 65, 37)
    _check(rfm, c, None, 0.3, k, f"k={k}")
    _check(rfm, c, c.penalty, 0.7, k, f"k={k} penalty")


def test_more_picks_than_candidates_pads(rfm):
    c = dc.case(dc.GPU_LISTS, 63, 5)
    items, scores, values, pos = _check(rfm, c, None, 0.7, 64, "k=64 of 63")
    assert (items[:, 63] == -1).all() and (pos[:, 63] == -1).all() and np.isnan(scores[:, 63]).all() and np.isnan(values[:, 63]).all()
    assert (np.sort(pos[:, :63], axis=1) == np.arange(63)[None, :]).all()


def test_candidate_rows_wider_than_the_depth(rfm):
    c = dc.case(dc.GPU_LISTS, 65, 37)
    for ld_c in (66, 68, 200):
        _check(rfm, c, c.penalty, 0.3, 9, f"ld_c={ld_c}", ld_c=ld_c, ld_R=40)


@pytest.mark.parametrize("penalty", [False, True])
@pytest.mark.parametrize("lam", dc.GPU_LAMBDAS)
def test_trade_offs(rfm, lam, penalty):
    """lambda = 0 without a penalty ties every candidate at step 0: held bitwise, as every exact tie."""
    c = dc.case(dc.GPU_LISTS, 65, 5)
    items, scores, values, pos = _check(rfm, c, c.penalty if penalty else None, lam, 9, f"lambda={lam} penalty={penalty}")
    if lam == 1.0 and not penalty:
        assert (pos == np.arange(9)[None, :]).all() and values.tobytes() == c.scores[:, :9].tobytes()
    if lam == 0.0 and not penalty:
        assert (items[:, 0] == c.items.max(axis=1)).all(), "all values equal: the highest id"


def test_list_counts_and_a_workgroup_s_second_list(rfm):
    rt = rfm[3]
    for n in (1, 2):
        c = dc.case(n, 65, 5)
        _check(rfm, c, None, 0.3, 9, f"lists={n}")
    cap = dc.geometry(10 ** 6, 9, 5, ctx=rt.ctx)["workgroups"]
    assert cap == _n_cu(rt) * 5
    n = cap + 1  # the smallest count that gives a workgroup (the first) its second list
    g = dc.geometry(n, 9, 5, k=3, ctx=rt.ctx)
    assert (g["workgroups"], g["passes"]) == (cap, 2)
    c = dc.case(n, 9, 5)
    got = _check(rfm, c, c.penalty, 0.7, 3, f"lists={n}", oracle=False)
    rows = [0, 1, cap - 1, cap]
    o = dc.select_oracle(c.items[rows], c.scores[rows], c.R, 5, c.penalty, 0.7, 3)
    dc.assert_against_oracle([a[rows] for a in got], o, c.scores[rows], f"lists={n}: first, last and second-pass rows")


def test_special_inputs(rfm):
    """Pads of -1 / NaN as rfm_pair_order leaves them, ids outside the table, a NaN score, a NaN row and
    an Inf row as candidate and as the chosen item, a repeated id: the statement's bytes (what the
    statement does with them: test_diverse_host.py)."""
    s = dc.special_case()
    for lam in (0.3, 0.7, 1.0, 0.0):
        for penalty in (None, s.penalty):
            items, _, _, pos = _check(rfm, s, penalty, lam, 64, f"special inputs lambda={lam} penalty={penalty is not None}",
                                      oracle=False)
            assert items.max() < s.n_items and not set(pos[0].tolist()) & (set(s.where["outside"]) | {s.where["nan_score"]}
                                                                           | set(s.where["padded"]))
    for kf in (1, 65, 400):
        _check(rfm, dc.special_case(kf), None, 0.5, 64, f"special inputs factors={kf}", oracle=False)
    # a list of nothing but pads
    empty = dc.special_case()
    empty.items, empty.scores = np.full((1, 65), -1, np.int32), np.full((1, 65), np.nan)
    items, scores, values, pos = _check(rfm, empty, None, 0.5, 9, "an empty list", oracle=False)
    assert (items == -1).all() and (pos == -1).all() and np.isnan(scores).all() and np.isnan(values).all()


def test_planted_twins_tie_exactly_and_the_higher_id_goes_first(rfm):
    tw = dc.twin_case()
    lo, hi = tw.twins
    items, scores, values, _ = _check(rfm, tw, None, 1.0, 9, "twins lambda=1", oracle=False)
    assert (items[:, 0] == hi).all() and (items[:, 1] == lo).all(), "adjacent picks, the higher id first"
    assert values[:, 0].tobytes() == values[:, 1].tobytes() and scores[:, 0].tobytes() == scores[:, 1].tobytes()
    for lam in (0.5, 0.0):
        items, _, _, _ = _check(rfm, tw, None, lam, 9, f"twins lambda={lam}", oracle=False)
        if lam == 0.5:
            assert (items[:, 0] == hi).all()


def test_same_bytes_twice(rfm):
    c = dc.case(dc.GPU_LISTS, 257, 37)
    a = dc.select(rfm, c.items, c.scores, c.R, 37, c.penalty, 0.3, 64)
    b = dc.select(rfm, c.items, c.scores, c.R, 37, c.penalty, 0.3, 64)
    dc.assert_same_bits(b, a, "the same call twice")


def test_refused_calls_leave_the_outputs_untouched(rfm):
    from relevance_factorizationmachine_amd import _lib
    c = dc.case(dc.GPU_LISTS, 65, 5)
    ok = dict(kf=5, penalty=None, lam=0.5, k=9)
    for bad in (dict(k=0), dict(k=65), dict(lam=-0.01), dict(lam=1.01), dict(lam=float("nan")), dict(kf=0), dict(kf=1025),
                dict(ld_c=64), dict(ld_R=4)):
        args = dict(ok)
        args.update(bad)
        assert dc.select(rfm, c.items, c.scores, c.R, args.pop("kf"), args.pop("penalty"), args.pop("lam"), args.pop("k"),
                         expect=_lib.RFM_ERR_BAD_ARG, **args) is None
        assert _lib.last_error()
    wide = np.zeros((1, 1025), np.int32)
    assert dc.select(rfm, wide, np.zeros((1, 1025)), c.R, 5, None, 0.5, 9, expect=_lib.RFM_ERR_BAD_ARG) is None
    rt = rfm[3]
    lib, buf = rt.lib, rt.upload(np.zeros(16))
    p = buf.data_ptr()
    good = [rt.ctx, p, p, 1, 1, 1, p, 1, 1, 1, None, 0.5, 1, p, p, p, p]
    for at in (0, 1, 2, 6, 13, 14, 15, 16):
        args = list(good)
        args[at] = None
        assert lib.rfm_diverse_select(*args) == _lib.RFM_ERR_BAD_ARG
    for at, value in ((3, -1), (7, 0), (7, 2 ** 31)):
        args = list(good)
        args[at] = value
        assert lib.rfm_diverse_select(*args) == _lib.RFM_ERR_BAD_ARG
    args = list(good)
    args[3] = 0  # no list: nothing to do, nothing launched
    assert lib.rfm_diverse_select(*args) == _lib.RFM_OK
    rt.sync()
    assert not buf.cpu().numpy().any()
