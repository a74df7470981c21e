"""Shared by the catalogue-rank tests (test_rank_items_host.py, test_gpu_rank_items.py): the NumPy
statement of the definition, the fixture's 14 models as logit matrices, the
held-out split of ``tests/golden/recommend.npz`` and the host oracle of the catalogue metrics.
Nothing here touches the GPU or the package under test."""
import warnings

import numpy as np

import recommend_common as rc
from oracle import cpu_ref

K_LIST = [1, 5, 9, 64, 100, 203]
METRICS = ["DCG", "Recall", "MAP", "MRR", "AUC"]
MODELS = [("fm", layout, k, alpha) for layout in rc.LAYOUTS for k, alpha in rc.FM_CASES] + [
    ("mf", None, k, None) for k in rc.MF_FACTORS]


def model_id(m):
    return f"{m[1]}-{rc.case_name(m[2], m[3])}" if m[0] == "fm" else f"mf-k{m[2]}"


def model_logits(g, gls, model):
    """NumPy logits ``[61, 203]`` of a fixture model; ``gls``: {layout: recommend_fm_<layout>.npz}."""
    kind, layout, k, alpha = model
    if kind == "mf":
        return rc.mf_logits(g[f"mf_k{k}_P"], g[f"mf_k{k}_Q"], g[f"mf_k{k}_bu"], g[f"mf_k{k}_bi"], float(g[f"mf_k{k}_b"]))
    w0, w, V = rc.fm_parameters(g, gls[layout], layout, k, alpha)
    return rc.fm_logits(*rc.side_matrices(layout, g["user_table"], g["item_table"], g["context"]), w0, w, V)


def ranks_by_definition(z, excluded=None):
    """``(ranks [n_items], n_candidates)`` of one user's logits ``z``: candidates = not NaN and not
    ``excluded`` (bool mask); rank of item i = number of candidates j != i with z[j] > z[i], or
    z[j] == z[i] and j > i; -1 where z[i] is NaN.  An excluded item is ranked against the candidates."""
    z = np.asarray(z, dtype=np.float64)
    idx = np.arange(z.shape[0])
    cand = ~np.isnan(z) if excluded is None else ~np.isnan(z) & ~np.asarray(excluded)
    with np.errstate(invalid="ignore"):
        better = (z[:, None] > z[None, :]) | ((z[:, None] == z[None, :]) & (idx[:, None] > idx[None, :]))  # [j, i]
    ranks = (better & cand[:, None]).sum(axis=0).astype(np.int32)
    ranks[np.isnan(z)] = -1
    return ranks, int(cand.sum())


def ranks_by_argsort(z):
    """Position of every item in ``np.argsort(z, kind="stable")[::-1]`` (no NaN, no exclusion)."""
    order = np.argsort(z, kind="stable")[::-1]
    pos = np.empty(z.shape[0], dtype=np.int32)
    pos[order] = np.arange(z.shape[0], dtype=np.int32)
    return pos


def min_relative_gap(Z):
    """Smallest gap between two neighbouring logits of one user, relative to the largest |logit|."""
    s = np.sort(Z, axis=1)
    return float(np.min(s[:, 1:] - s[:, :-1]) / np.max(np.abs(Z)))


def heldout(g):
    """``(train mask [61, 203], positives (users, items), dropped (users, items))``: train pairs =
    the fixture's fitted rows, positives = the later rows with label 1 that are not train pairs,
    dropped = those that are."""
    n, NI = int(g["n_log"]), rc.N_ITEMS
    u, i, y = g["log_users"].astype(np.int64), g["log_items"].astype(np.int64), g["labels"]
    train = np.zeros((rc.N_USERS, NI), dtype=bool)
    train[u[:n], i[:n]] = True
    pos = np.unique((u[n:] * NI + i[n:])[y[n:] == 1])
    seen = train[pos // NI, pos % NI]
    return train, (pos[~seen] // NI, pos[~seen] % NI), (pos[seen] // NI, pos[seen] % NI)


def oracle_metrics(Z, positives, excluded, K=K_LIST):
    """The catalogue metrics with the oracle's ``test_metrics`` (the reference's ``TestEvaluator``)
    on the frame of ALL candidate pairs of the users that have a positive -- label 1 for the
    positives, pscore ones, scores = logits -- and MRR / AUC stated directly."""
    pu, pi = positives
    label = np.zeros(Z.shape)
    label[pu, pi] = 1.0
    users = np.unique(pu)
    fu, fi = [], []
    for u in users:
        items = np.flatnonzero(~excluded[u] & ~np.isnan(Z[u]))
        fu.append(np.full(items.shape[0], u))
        fi.append(items)
    fu, fi = np.concatenate(fu), np.concatenate(fi)
    frame = {"user": fu, "item": fi, "label": label[fu, fi], "pscore": np.ones(fu.shape[0])}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore", category=RuntimeWarning)  # ME (not used) of a K no user reaches
        out = cpu_ref.test_metrics(frame, Z[fu, fi], K=tuple(K), used_metrics=("DCG", "Recall", "MAP"), n_items=Z.shape[1])
    mrr, auc = [], []
    for u in users:
        items = np.flatnonzero(~excluded[u] & ~np.isnan(Z[u]))
        z, y = Z[u, items], label[u, items]
        order = np.argsort(z, kind="stable")[::-1]
        mrr.append(1.0 / (1.0 + np.flatnonzero(y[order] == 1)[0]))
        p, n = z[y == 1], z[y == 0]
        # share of (positive, non-positive candidate) pairs ordered correctly; equal logits go by
        # the item index, as everywhere
        ip, im = items[y == 1], items[y == 0]
        right = (p[:, None] > n[None, :]) | ((p[:, None] == n[None, :]) & (ip[:, None] > im[None, :]))
        auc.append(right.mean() if n.size else np.nan)
    return {"DCG": out["DCG"], "Recall": out["Recall"], "MAP": out["MAP"], "MRR": [float(np.nanmean(mrr))],
            "AUC": [float(np.nanmean(auc))]}


def assert_metrics_equal(got, want, what, rtol=1e-12):
    for m in METRICS:
        a, b = np.asarray(got[m], dtype=np.float64), np.asarray(want[m], dtype=np.float64)
        print(what, m, a, b)
        assert a.shape == b.shape, (what, m)
        assert np.all(np.abs(a - b) <= rtol * np.abs(b)), (what, m, a, b)
