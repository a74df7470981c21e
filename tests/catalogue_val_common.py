"""Shared by the tests of the per-iteration catalogue metrics (DESIGN.md 8 N8;
test_catalogue_val_host.py, test_gpu_catalogue_val.py): synthetic grouped ranks with their host
answer, and the fixture log of ``tests/golden/recommend*.npz`` as ``fit()`` inputs.  Nothing here
touches the GPU."""
import numpy as np

import rank_items_common as rk
import recommend_common as rc

ABI_K = [1, 5, 64, 100, 10_000]
POSITIVES_PER_USER = (1, 2, 63, 64, 65, 130, 300)
N_ITERS = 8


def synthetic_ranks(n_users, seed, rank0="mixed", all_dropped=False):
    """Grouped targets of ``n_users`` users with the edge cases of the kernel: positives per user
    drawn from ``POSITIVES_PER_USER``, distinct ranks per user out of 0..C-1, some at -1, (from two
    users on) one user with every positive at -1 and one with C == P.  ``rank0``: "mixed" leaves the
    draw alone, "present" puts rank 0 into every user, "absent" into none.  Returns ``(indptr int64,
    ranks int32, candidates int32, weights float64)``."""
    rng = np.random.default_rng(seed)
    counts = rng.choice(POSITIVES_PER_USER, size=n_users)
    counts[0] = POSITIVES_PER_USER[seed % len(POSITIVES_PER_USER)]
    indptr = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    ranks, cand = [], []
    for s, P in enumerate(counts):
        C = int(P + rng.integers(1, 4 * P + 20000 // P))
        if n_users > 1 and s == n_users - 1:
            C = int(P)  # every candidate is a positive: no AUC
        lo = 0 if C == P or rank0 != "absent" else 1
        r = rng.choice(np.arange(lo, C), size=P, replace=False) if C - lo >= P else np.arange(C)
        if rank0 == "present" and 0 not in r:
            r[rng.integers(0, P)] = 0
        if C > P:
            r[rng.random(P) < 0.1] = -1  # a NaN logit
        if all_dropped or (n_users > 1 and s == n_users // 2):
            r[:] = -1
        ranks.append(r)
        cand.append(C)
    weights = 1.0 / rng.uniform(0.05, 1.0, size=int(indptr[-1]))
    return indptr, np.concatenate(ranks).astype(np.int32), np.asarray(cand, dtype=np.int32), weights


def host_answer(indptr, ranks, cand, weights, K):
    """``(metrics, weighted DCG@K, counts)`` on the host: ``CatalogueEvaluator.metrics`` (pinned to
    the oracle by test_rank_items_host.py), the weighted DCG as the direct sum over the ranked
    positives, and (users counted, users counted for the AUC, unranked positives)."""
    from relevance_factorizationmachine_amd.evaluate import CatalogueEvaluator

    n_sel = indptr.shape[0] - 1
    users = np.repeat(np.arange(n_sel), np.diff(indptr))
    ev = CatalogueEvaluator((np.zeros(0, np.int64), np.zeros(0, np.int64)), 1, K, rk.METRICS)
    want = ev.metrics(users, ranks, np.repeat(cand, np.diff(indptr)))
    dcg, n_users, n_auc = [], 0, 0
    for s in range(n_sel):
        r, v = ranks[indptr[s]:indptr[s + 1]].astype(np.float64), weights[indptr[s]:indptr[s + 1]]
        v, r = v[r >= 0], r[r >= 0]
        if r.size == 0:
            continue
        n_users += 1
        n_auc += int(cand[s] > r.size)
        order = np.argsort(r)
        r, v = r[order], v[order]
        g = np.where(r == 0, 1.0, 1.0 / np.log2(np.maximum(r, 1.0) + 1.0))
        dcg.append([float(np.sum((v * g)[r < k])) for k in K])
    wdcg = np.mean(np.asarray(dcg).reshape(-1, len(K)), axis=0) if dcg else np.full(len(K), np.nan)
    return want, wdcg, (n_users, n_auc, int(np.count_nonzero(ranks < 0)))


def fixture_split(g, layout=None):
    """``(train, val)`` of the fixture log as ``fit()`` takes them: the first ``n_log`` rows and
    the rest; FM design matrix of ``layout``, or MF's (user, item) pairs when it is None."""
    n = int(g["n_log"])
    if layout is None:
        X = np.stack([g["log_users"], g["log_items"]], axis=1)
    else:
        XU, XI = rc.side_matrices(layout, g["user_table"], g["item_table"], g["context"])
        X = rc.pair_rows(XU, XI, g["log_users"], g["log_items"])
    cut = lambda a, b: {"features": X[a:b], "labels": g["labels"][a:b], "pscores": g["pscores"][a:b]}  # noqa: E731
    return cut(0, n), cut(n, X.shape[0])


def row(history, e):
    """Row ``e`` of a ``history`` as ``{metric: 1-d array}``."""
    return {m: np.asarray(v[e], dtype=np.float64) for m, v in history.items()}


def assert_same_bits(a, b, what):
    """Two ``{metric: values}`` (a ``history`` row, an ``evaluate()`` result) bit for bit; NaN
    equals NaN."""
    assert set(a) == set(b) == set(rk.METRICS), what
    for m in rk.METRICS:
        x, y = np.asarray(a[m], dtype=np.float64), np.asarray(b[m], dtype=np.float64)
        assert x.shape == y.shape and x.tobytes() == y.tobytes(), (what, m, x, y)
