#!/usr/bin/env python3
"""Ranks of given (user, item) pairs against the whole catalogue, two ways, in one process:

  R  `model.rank_items(...)`: side sums + two passes of the pair tile on the f64
     matrix core (the targets' logits, then the counting) + the finish; timed as the public call
     (grouping on the host, uploads, the download of the ranks) and as the grouped device call
     alone (`recommend._rank_grouped`: uploads of the target lists + the launches + the download);
  P  what the package could do before: `score_pairs()` to the host (the dense [users, items]
     matrix of PROBABILITIES) + a stable argsort per user in NumPy for the ranks of the same
     targets.  Not the same answer where probabilities saturate to exactly 0.0 / 1.0 (the share of
     such entries and of the targets whose rank differs is printed); the logit ranks are R's.

Targets: 10 and 100 random items per user, and at the small shape every item of every user (the
worst case for the counting, whose work is users x items x targets-per-user comparisons).

Device-synchronised host clock, every path warmed up once, REPEATS timed runs each (min / median /
max printed: the spread of the same command).

usage (GPU box): python tests/manual/rank_items_timing.py [--device-only] [--repeats N]
`--device-only` runs, per configuration, `score_pairs`' launch and the grouped device call alone,
CALLS times each: the run to put under `rocprofv3 --kernel-trace --stats`
(profiles/rank_items_prof.sh), where the kernel time of `pair_tile_kernel<0>` (rfm_pair_scores) is
the floor of one pass over the product."""
import argparse
import os
import sys
import time

import numpy as np
from scipy import sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from relevance_factorizationmachine_amd import _lib, features, recommend, synth  # noqa: E402

SHAPES = (("kuairec_small", 1411, 3327), ("kuairec_big", 7176, 10728))
FACTORS = (32, 400)
TARGETS = (10, 100)
CALLS = 3  # --device-only: launches of every kind per configuration (profiles/rank_items_trace_summary.py)


def tables(rng, nu, ni):
    user = np.hstack([np.eye(s)[rng.integers(0, s, size=nu)] for s in synth.KUAIREC_USER_GROUPS])
    item = np.hstack([rng.standard_normal((ni, 4)),
                      np.eye(synth.KUAIREC_N_TAGS)[rng.integers(0, synth.KUAIREC_N_TAGS, size=ni)]])
    return sp.csr_matrix(user), sp.csr_matrix(item), sp.csr_matrix(rng.standard_normal((nu, 1)))


def clock(fn, rt, repeats, warm=True):
    if warm:
        fn()  # warm-up: library load, kernels, allocator pools
    rt.sync()
    out = []
    for _ in range(repeats):
        rt.sync()
        t0 = time.perf_counter()
        fn()
        rt.sync()
        out.append(1e3 * (time.perf_counter() - t0))
    return np.array(out)


def show(label, ms):
    print(f"  {label}: {np.median(ms):10.2f} ms (min {ms.min():.2f}, max {ms.max():.2f}, {len(ms)} runs)", flush=True)
    return float(np.median(ms))


def targets(rng, nu, ni, per_user):
    if per_user >= ni:
        return np.repeat(np.arange(nu), ni), np.tile(np.arange(ni), nu)
    items = np.stack([rng.choice(ni, size=per_user, replace=False) for _ in range(nu)])
    return np.repeat(np.arange(nu), per_user), items.ravel()


def host_ranks(S, users, items):
    """Ranks of the targets from the dense score matrix: one stable argsort per user."""
    ranks = np.empty(users.shape[0], dtype=np.int32)
    pos = np.empty(S.shape[1], dtype=np.int32)
    at = 0
    for u in range(S.shape[0]):
        n = int(np.searchsorted(users, u, side="right")) - at
        if n:
            pos[np.argsort(S[u], kind="stable")[::-1]] = np.arange(S.shape[1], dtype=np.int32)
            ranks[at:at + n] = pos[items[at:at + n]]
        at += n
    return ranks


def run(name, label, nu, ni, operands, n_factors, rank_items, score_pairs, rt, args):
    rng = np.random.default_rng(5)
    A, LU, B, LI, c = operands()
    print(f"{name} {nu} x {ni}, {label}", flush=True)
    if args.device_only:
        import torch
        out = rt.empty((nu, ni), torch.float64)
        for _ in range(CALLS):
            _lib.check(rt.lib.rfm_pair_scores(rt.ctx, A.data_ptr(), LU.data_ptr(), nu, None, nu, B.data_ptr(),
                                              LI.data_ptr(), ni, n_factors, c.data_ptr(), out.data_ptr()))
        rt.sync()
        del out
    per_user = TARGETS + ((ni,) if name == "kuairec_small" else ())
    for t in per_user:
        users, items = targets(rng, nu, ni, t)
        sel, indptr, tgt, _ = recommend.group_pairs(users, items, nu, ni)
        grouped = lambda: recommend._rank_grouped(rt, A, LU, B, LI, c, n_factors, sel, indptr, tgt, None)  # noqa: E731
        what = "every item" if t >= ni else f"{t} targets per user"
        if args.device_only:
            for _ in range(CALLS):
                grouped()
            continue
        r_ms = show(f"R rank_items(), {what}", clock(lambda: rank_items(users, items), rt, args.repeats))
        show(f"R grouped device call alone, {what}", clock(grouped, rt, args.repeats))
        if t != TARGETS[-1]:
            continue
        big = nu * ni > 2e7
        p_ms = show(f"P score_pairs() to the host + NumPy argsort per user, {what}",
                    clock(lambda: host_ranks(score_pairs(), users, items), rt, 1 if big else max(2, args.repeats // 2),
                          warm=not big))
        S = score_pairs()
        differ = float(np.mean(host_ranks(S, users, items) != rank_items(users, items)[0]))
        print(f"  P / R = {p_ms / r_ms:.1f}; probabilities exactly 0.0 or 1.0: {100 * np.mean((S == 0.0) | (S == 1.0)):.2f} %, "
              f"targets whose rank from the probabilities differs from the logit rank: {100 * differ:.2f} %", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import relevance_factorizationmachine_amd as pkg

    for name, nu, ni in SHAPES:
        user, item, ctx = tables(np.random.default_rng(1), nu, ni)
        for k in FACTORS:
            model = pkg.FactorizationMachines(estimator="IPS", n_epochs=1, n_factors=k, lr=1e-4, batch_size=1, seed=7,
                                              n_features=synth.n_features_of(synth.SHAPES[name]), alpha=2.0)
            sides = features.sides_kuairec(model._rt, nu, ni, ctx, user, item)
            run(name, f"FM k = {k}, alpha = 2.0", nu, ni, lambda: recommend.operands(model, sides)[1:6], k,
                lambda u, i: model.rank_items(sides, u, i), lambda: model.score_pairs(sides), model._rt, args)
        # MF at k = 400: P, Q as they are initialised, b as fit() would set it
        mf = pkg.LogisticMatrixFactorization(estimator="IPS", n_epochs=1, n_factors=400, n_users=nu, n_items=ni, lr=0.02,
                                             reg=0.5, batch_size=1, seed=7)
        mf.b = 0.5
        run(name, "MF k = 400", nu, ni, lambda: recommend.operands(mf)[1:6], 400, mf.rank_items, mf.score_pairs, mf._rt, args)


if __name__ == "__main__":
    main()
