"""Deep ranking of the catalogue, the part that needs no GPU: the workspace sizes
of ``rfm_pair_order``, the argument checks of ``recommend.rank_catalogue`` that come before any
device call, and the metric arithmetic of ``CatalogueExposure`` against the oracle's
``test_metrics`` (the reference's ``TestEvaluator``) on the frame of all candidate pairs."""
import numpy as np
import pytest

import rank_catalogue_common as rcc
import rank_items_common as rk

NU, NI = rcc.NU, rcc.NI


# --------------------------------------------------------------------------- 1
def test_order_workspace_sizes():
    from relevance_factorizationmachine_amd import recommend

    for depth in (0, -3):
        with pytest.raises(ValueError, match="depth"):
            recommend.order_workspace_bytes(61, 203, depth)
    for depth in (2.0, "3", None, True):
        with pytest.raises(ValueError, match="integer"):
            recommend.order_workspace_bytes(61, 203, depth)
    with pytest.raises(ValueError):
        recommend.order_workspace_bytes(61, 0, 5)
    with pytest.raises(ValueError):
        recommend.order_workspace_bytes(-1, 203, 5)
    for n_sel in (0, 1, 61, 64, 65, 200, 7176):
        for depth in (1, 64, 65, 5000, 1 << 40):
            small, mid, large = (recommend.order_workspace_bytes(n_sel, ni, depth) for ni in (1, 203, 10728))
            for lo, hi in (small, mid, large):
                assert 0 < lo <= hi
            assert small[0] < mid[0] < large[0] and small[1] < mid[1] < large[1]  # both grow with n_items
            assert mid[0] >= 64 * 203 * 8  # a block of 64 users' logits
            assert mid[1] >= max(n_sel, 1) * 203 * 8
    # the minimum is one block of 64 users whatever the selection; the preferred size follows it
    assert recommend.order_workspace_bytes(1, 203, 9)[0] == recommend.order_workspace_bytes(7176, 203, 9)[0]
    assert recommend.order_workspace_bytes(64, 203, 9)[1] < recommend.order_workspace_bytes(65, 203, 9)[1]
    # the default cap of rank_catalogue is never below the minimum it is raised to
    assert recommend.ORDER_WORKSPACE_BYTES >= recommend.order_workspace_bytes(7176, 10728, 10728)[1]


class _Shape:
    def __init__(self, n):
        self.shape = (n, 4)


def test_rank_catalogue_rejects_bad_arguments_before_any_device_call():
    from relevance_factorizationmachine_amd import recommend

    def call(depth, **kw):  # rt = None: anything that reached the device would raise AttributeError
        return recommend.rank_catalogue(None, _Shape(7), None, _Shape(11), None, None, 4, depth, **kw)

    for depth in (0, -1):
        with pytest.raises(ValueError, match="at least 1"):
            call(depth)
    for depth in (2.5, "3", None, True, np.float64(4.0)):
        with pytest.raises(ValueError, match="integer"):
            call(depth)
    with pytest.raises(ValueError, match="user id"):
        call(3, users=[0, 7])
    with pytest.raises(ValueError, match="user id"):
        call(3, users=[-1])
    with pytest.raises(ValueError, match="1-d"):
        call(3, users=[[0]])
    with pytest.raises(ValueError, match="1-d"):
        call(3, users=[0.5])


# --------------------------------------------------------------------------- 2
@pytest.mark.parametrize("model", rcc.MODELS, ids=rcc.model_id)
def test_exposure_arithmetic_matches_the_oracle_on_all_candidate_pairs(model):
    from relevance_factorizationmachine_amd.evaluate import CatalogueExposure

    Z, train, ps = rcc.logits(model), rcc.train_mask(), rcc.item_pscores()
    gap = rk.min_relative_gap(Z)
    print(rcc.model_id(model), "smallest relative gap between neighbouring logits of a user:", gap)
    assert gap >= 4e-9  # the order is unambiguous: the oracle's unstable argsort has one answer
    for excluded in (train, None):
        items, _, n_ranked = rcc.expected_lists(Z, max(rcc.K_LIST), excluded)
        if excluded is not None:
            print("candidates per user:", n_ranked.min(), "..", n_ranked.max())
            assert 158 <= n_ranked.min() and n_ranked.max() <= 182  # K = 203 is all padding, 100 is not
            assert (items[:, 202] == -1).all() and (items[:, 99] >= 0).all()
        ev = CatalogueExposure(NI, rcc.K_LIST, rcc.METRICS, item_pscores=ps)
        got = ev.metrics(items)
        want = rcc.fixture_oracle(model, excluded is not None)
        rcc.assert_exposure_equal(got, want, rcc.model_id(model))
        if excluded is not None:
            assert np.isnan(got["ME"][-1]) and np.isnan(want["ME"][-1])  # ME@203: no user has 203 candidates
        # lists cut short of max(K) are lists padded with -1
        short = CatalogueExposure(NI, rcc.K_LIST, rcc.METRICS, item_pscores=ps).metrics(items[:, :182])
        if excluded is not None:
            rcc.assert_exposure_equal(short, want, rcc.model_id(model) + " short")


def test_exposure_small_cases_and_constructor_errors():
    from relevance_factorizationmachine_amd.evaluate import CatalogueExposure

    ps = np.array([0.5, 0.25, 1.0, 0.125])
    lists = np.array([[3, 1, 0, -1], [3, 0, -1, -1], [-1, -1, -1, -1]])
    ev = CatalogueExposure(4, [1, 2, 3, 4, 9], ["ME", "CatalogCoverage", "Gini"], item_pscores=ps)
    got = ev.metrics(lists)
    assert got["ME"][:3] == [0.125, (0.25 + 0.5) / 2, 0.5] and np.isnan(got["ME"][3]) and np.isnan(got["ME"][4])
    assert got["CatalogCoverage"] == [0.25, 0.75, 0.75, 0.75, 0.75]
    # frequencies at k = 2: item 3 twice, items 0 and 1 once, item 2 never -> sorted 0 1 1 2
    assert got["Gini"][1] == pytest.approx((-3 * 0 - 1 * 1 + 1 * 1 + 3 * 2) / (4 * 4), rel=1e-15)
    assert list(got) == ["ME", "CatalogCoverage", "Gini"]
    only = CatalogueExposure(4, [2], ["CatalogCoverage"]).metrics(lists)  # no pscores needed
    assert only == {"CatalogCoverage": [0.75]}
    with pytest.raises(ValueError, match="unknown metric"):
        CatalogueExposure(4, [1], ["DCG"], item_pscores=ps)
    with pytest.raises(ValueError, match="item_pscores"):
        CatalogueExposure(4, [1], ["ME"])
    with pytest.raises(ValueError, match="positive integers"):
        CatalogueExposure(4, [1, 0], ["Gini"])
    with pytest.raises(ValueError, match="positive integers"):
        CatalogueExposure(4, [], ["Gini"])
    with pytest.raises(ValueError, match="shape"):
        CatalogueExposure(4, [1], ["ME"], item_pscores=np.ones(5))
    with pytest.raises(ValueError, match="shape"):
        CatalogueExposure(4, [1], ["Gini"], item_pscores=np.ones((4, 1)))
