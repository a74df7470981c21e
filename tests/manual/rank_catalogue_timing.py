#!/usr/bin/env python3
"""Every user's ranking of the catalogue to a depth, three ways, in one process:

  D  `model.rank_catalogue(depth)`: side sums + the pair tile storing raw logits
     + one ranking workgroup per user (+ further pages beyond 4 096 ranks); timed as the public
     call (uploads, launches, the download of [users, depth] items and scores) and as the device
     call alone (`rfm_pair_order` on operands and outputs that stay in HBM);
  T  `model.recommend(k=64)` of the same build: one pass over the product plus a ranking, the
     floor, and all the package could return before;
  P  the only route past 64 before: `score_pairs()` to the host (the dense [users, items] matrix
     of PROBABILITIES) + a stable argsort per user in NumPy.  Not the same answer where
     probabilities saturate to exactly 0.0 / 1.0: the share of such entries and of the first 100
     positions that differ from D's is printed; the logit order is D's.

Depths: 100, 1 000 and the whole catalogue.  Device-synchronised host clock, every path warmed up
once, REPEATS timed runs each (min / median / max printed: the spread of the same command).

usage (GPU box): python tests/manual/rank_catalogue_timing.py [--device-only PLAN.json] [--repeats N]
`--device-only` runs, per configuration, `rfm_pair_topk` at k = 64 and `rfm_pair_order` at every
depth, CALLS times each, and writes the order of the launches to PLAN.json: the run to put under
`rocprofv3 --kernel-trace --stats` (profiles/rank_catalogue_prof.sh)."""
import argparse
import json
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
DEPTHS = (100, 1000, None)  # None: the whole catalogue
CALLS = 3
PAGE = 4096  # ranks of a page (kOrderMaxP of csrc/rfm_pairs.hip)


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


def device_calls(rt, operands, n_factors, nu, ni):
    """``(topk64(), order(depth))``: the two ABI calls on buffers that stay on the device."""
    import torch
    A, LU, B, LI, c = operands
    head = (rt.ctx, A.data_ptr(), LU.data_ptr(), nu, None, nu, B.data_ptr(), LI.data_ptr(), ni, n_factors,
            c.data_ptr(), None, None)
    ws_t = rt.empty((recommend.topk_workspace_bytes(nu, ni, 64),), torch.uint8)
    it_t, sc_t = rt.empty((nu, 64), torch.int32), rt.empty((nu, 64), torch.float64)
    nbytes = min(recommend.order_workspace_bytes(nu, ni, 1)[1], recommend.ORDER_WORKSPACE_BYTES)
    ws_o = rt.empty((nbytes,), torch.uint8)
    n_ranked = rt.empty((nu,), torch.int32)
    outs = {}

    def topk64():
        _lib.check(rt.lib.rfm_pair_topk(*head, 64, ws_t.data_ptr(), it_t.data_ptr(), sc_t.data_ptr()))

    def order(depth):
        if depth not in outs:
            outs[depth] = rt.empty((nu, depth), torch.int32), rt.empty((nu, depth), torch.float64)
        it, sc = outs[depth]
        _lib.check(rt.lib.rfm_pair_order(*head, depth, ws_o.data_ptr(), nbytes, it.data_ptr(), sc.data_ptr(),
                                         n_ranked.data_ptr()))

    return topk64, order


def run(name, label, nu, ni, operands, n_factors, model_calls, rt, args, plan):
    rank_catalogue, recommend_64, score_pairs = model_calls
    print(f"{name} {nu} x {ni}, {label}", flush=True)
    topk64, order = device_calls(rt, operands(), n_factors, nu, ni)
    depths = [d or ni for d in DEPTHS]
    if args.device_only:
        for _ in range(CALLS):
            topk64()
        rt.sync()
        plan.append({"config": f"{name} {label}", "what": "rfm_pair_topk k=64", "calls": CALLS, "tile": 1, "rank": 1})
        for depth in depths:
            for _ in range(CALLS):
                order(depth)
            rt.sync()
            plan.append({"config": f"{name} {label}", "what": f"rfm_pair_order depth {depth}", "calls": CALLS,
                         "tile": 1, "rank": -(-min(depth, ni) // PAGE)})
        return
    t_ms = show("T recommend(k=64)", clock(recommend_64, rt, args.repeats))
    show("T rfm_pair_topk k=64 alone", clock(topk64, rt, args.repeats))
    for depth in depths:
        d_ms = show(f"D rank_catalogue(depth={depth})", clock(lambda: rank_catalogue(depth), rt, args.repeats))
        show(f"D rfm_pair_order depth {depth} alone", clock(lambda: order(depth), rt, args.repeats))
        print(f"  D / T = {d_ms / t_ms:.2f}", flush=True)
    big = nu * ni > 2e7

    def host_order():
        S = score_pairs()
        return S, np.stack([np.argsort(S[u], kind="stable")[::-1] for u in range(S.shape[0])])

    p_ms = show("P score_pairs() to the host + a stable NumPy argsort per user (whole catalogue)",
                clock(host_order, rt, 1 if big else max(2, args.repeats // 2), warm=not big))
    S, by_probability = host_order()
    items = rank_catalogue(100)[0]
    print(f"  P / D(whole catalogue) = {p_ms / d_ms:.1f}; probabilities exactly 0.0 or 1.0: "
          f"{100 * np.mean((S == 0.0) | (S == 1.0)):.2f} %, first-100 positions where the order of the probabilities "
          f"differs from the logit order: {100 * np.mean(by_probability[:, :100] != items):.2f} %", flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device-only", metavar="PLAN.json", default=None)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import relevance_factorizationmachine_amd as pkg

    plan = []
    for name, nu, ni in SHAPES:
        user, item, ctx = tables(np.random.default_rng(1), nu, ni)
        for k in FACTORS:
            model = pkg.FactorizationMachines(estimator="IPS", n_epochs=1, n_factors=k, lr=1e-4, batch_size=1, seed=7,
                                              n_features=synth.n_features_of(synth.SHAPES[name]), alpha=2.0)
            sides = features.sides_kuairec(model._rt, nu, ni, ctx, user, item)
            run(name, f"FM k = {k}, alpha = 2.0", nu, ni, lambda: recommend.operands(model, sides)[1:6], k,
                (lambda d: model.rank_catalogue(sides, d), lambda: model.recommend(sides, 64),
                 lambda: model.score_pairs(sides)), model._rt, args, plan)
        # MF at k = 400: P, Q as they are initialised, b as fit() would set it
        mf = pkg.LogisticMatrixFactorization(estimator="IPS", n_epochs=1, n_factors=400, n_users=nu, n_items=ni, lr=0.02,
                                             reg=0.5, batch_size=1, seed=7)
        mf.b = 0.5
        run(name, "MF k = 400", nu, ni, lambda: recommend.operands(mf)[1:6], 400,
            (mf.rank_catalogue, lambda: mf.recommend(64), mf.score_pairs), mf._rt, args, plan)
    if args.device_only:
        with open(args.device_only, "w") as f:
            json.dump(plan, f, indent=1)


if __name__ == "__main__":
    main()
