"""The documented tie rule of ``rfm_val_dcg`` restated on the host (test_gpu_eval.py,
dp_peers_common.py): among equal scores the later row ranks first, which is the order
``argsort(kind="stable")[::-1]`` gives.  NumPy and the oracle only; no GPU import."""
import numpy as np

from oracle import cpu_ref


def stable_rule_dcg(frame, scores, pscores, k):
    """IPS-DCG@k with the documented tie rule (later row first), per user."""
    vals, ok = [], []
    for rows in cpu_ref._per_user_slices(frame["user"]):
        rank = np.argsort(scores[rows], kind="stable")[::-1]
        ys = frame["label"][rows][rank]
        if np.sum(ys) == 0:
            vals.append(0.0)
            ok.append(False)
            continue
        vals.append(cpu_ref.ips_dcg_at_k(ys, k, pscores[rows][rank]))
        ok.append(True)
    return np.array(vals), np.array(ok)


def order_dependent_users(frame, scores, pscores, k):
    """Users (with a positive label) for whom a score tie between rows of different label or
    propensity reaches into the first k ranks."""
    flags = []
    for rows in cpu_ref._per_user_slices(frame["user"]):
        if np.sum(frame["label"][rows]) == 0:
            flags.append(False)
            continue
        rank = np.argsort(scores[rows], kind="stable")[::-1]
        sc, ys, ps = scores[rows][rank], frame["label"][rows][rank], pscores[rows][rank]
        top = sc[: min(k, len(sc))]
        flag = bool(np.isnan(sc).any())
        for v in np.unique(top[~np.isnan(top)]):
            m = sc == v
            flag = flag or len(set(zip(ys[m].tolist(), ps[m].tolist()))) > 1
        flags.append(flag)
    return np.array(flags)
