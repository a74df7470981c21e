"""Shared by the deep-ranking tests (test_rank_catalogue_host.py, test_gpu_rank_catalogue.py): the
NumPy statement of ``rank_catalogue``, the fixture's 14 models as logit matrices
(computed once per process and shared read-only) and the host oracle of the exposure metrics.
Nothing here touches the GPU or the package under test."""
import functools
import warnings

import numpy as np

import rank_items_common as rk
import recommend_common as rc
from conftest import load_golden
from oracle import cpu_ref

MODELS, model_id = rk.MODELS, rk.model_id
K_LIST = (1, 9, 64, 100, 203)
METRICS = ("ME", "CatalogCoverage", "Gini")
NU, NI = rc.N_USERS, rc.N_ITEMS


@functools.lru_cache(maxsize=None)
def gold():
    return load_golden("recommend"), {layout: load_golden(f"recommend_fm_{layout}") for layout in rc.LAYOUTS}


@functools.lru_cache(maxsize=None)
def fm_parameters(layout, k, alpha):
    """``w0, w, V`` of an FM fixture case (k = 400 is refitted by the oracle: once per process)."""
    g, gls = gold()
    return rc.fm_parameters(g, gls[layout], layout, k, alpha)


@functools.lru_cache(maxsize=None)
def logits(model):
    """``rk.model_logits`` of a fixture model, ``[61, 203]``, read-only."""
    g, gls = gold()
    kind, layout, k, alpha = model
    if kind == "mf":
        Z = rk.model_logits(g, gls, model)
    else:
        Z = rc.fm_logits(*rc.side_matrices(layout, g["user_table"], g["item_table"], g["context"]),
                         *fm_parameters(layout, k, alpha))
    Z.setflags(write=False)
    return Z


@functools.lru_cache(maxsize=None)
def train_mask():
    """The fixture's train pairs, bool ``[61, 203]``, read-only."""
    M = rk.heldout(gold()[0])[0]
    M.setflags(write=False)
    return M


def item_pscores(n_items=NI):
    """A propensity per item, as the reference's KuaiRec loader derives one from the item."""
    return np.random.default_rng(2024).uniform(0.05, 1.0, size=n_items)


def expected_lists(Z, depth, excluded=None, users=None):
    """The definition in NumPy: per selected user the stable descending argsort of the logits
    (equal logits: higher item index first) with the NaNs and the ``excluded`` items (bool mask by
    user id) taken out, cut at ``depth`` and padded with -1 / NaN.
    ``(items int32 [n, depth], logits float64 [n, depth], n_ranked int32 [n])``."""
    Z = np.asarray(Z, dtype=np.float64)
    users = np.arange(Z.shape[0]) if users is None else np.asarray(users)
    items = np.full((users.shape[0], depth), -1, dtype=np.int32)
    picked = np.full((users.shape[0], depth), np.nan)
    n_ranked = np.zeros(users.shape[0], dtype=np.int32)
    for s, u in enumerate(users):
        order = np.argsort(Z[u], kind="stable")[::-1]
        keep = ~np.isnan(Z[u][order])
        if excluded is not None:
            keep &= ~np.asarray(excluded)[u][order]
        order = order[keep]
        n_ranked[s] = order.shape[0]
        top = order[:depth]
        items[s, : top.shape[0]] = top
        picked[s, : top.shape[0]] = Z[u, top]
    return items, picked, n_ranked


def exposure_oracle(Z, excluded, pscores, K=K_LIST):
    """The oracle's ``test_metrics`` (the reference's ``TestEvaluator``) on the frame of ALL
    candidate pairs: label all ones (every user counts), pscore = the item's, scores = logits."""
    cand = ~np.isnan(Z) if excluded is None else ~np.isnan(Z) & ~np.asarray(excluded)
    fu, fi = np.nonzero(cand)
    frame = {"user": fu, "item": fi, "label": np.ones(fu.shape[0]), "pscore": np.asarray(pscores)[fi]}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)  # ME at a K that no user reaches
        return cpu_ref.test_metrics(frame, Z[fu, fi], K=tuple(K), used_metrics=("CatalogCoverage", "Gini"),
                                    n_items=Z.shape[1])


@functools.lru_cache(maxsize=None)
def fixture_oracle(model, with_exclusion):
    return exposure_oracle(logits(model), train_mask() if with_exclusion else None, item_pscores())


def assert_exposure_equal(got, want, what, rtol=1e-12):
    for m in METRICS:
        a, b = np.asarray(got[m], dtype=np.float64), np.asarray(want[m], dtype=np.float64)
        print(what, m, a, b)
        assert a.shape == b.shape, (what, m)
        np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=f"{what} {m}")
        ok = ~np.isnan(b)
        assert np.all(np.abs(a[ok] - b[ok]) <= rtol * np.abs(b[ok])), (what, m, a, b)
