#!/usr/bin/env python3
"""Top-9 of the whole catalogue for every user, two ways, alternated in one process:

  A  what the package could do before `recommend`: the design matrix of every (user, item) pair of
     a block of users (`features.fm_features_kuairec`) -> the forward over its rows (what
     `predict()` launches; the scores stay on the device) -> `rfm_topk_users`, K = 9; blocks of
     users sized to keep the pairs' CSR under about 1.5 GB;
  B  `model.recommend(sides, k=9)`: side sums + the pair tile on the f64 matrix core + the merge.

Device-synchronised host clock, every path warmed up once, REPEATS timed runs each (min / median /
max printed: the spread of the same command).  At the big shape path A is timed on the first
A_BLOCKS user blocks and scaled to all of them (printed as "extrapolated").  The two paths'
probabilities of the first user block are compared at the bounds of tests/test_gpu_recommend.py
(norm-wise 1e-9, element-wise 1e-5 |b| + 1e-12), and their top-9 lists item by item.

usage (GPU box): python tests/manual/recommend_timing.py [--only-b] [--repeats N]
`--only-b` runs path B alone (FM and MF): the run to put under `rocprofv3 --kernel-trace --stats`
for the kernels' own times; the achieved f64 FLOP/s of the tile kernel is
2 n_users n_items kpad / its time."""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np
from scipy import sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import assert_elementwise, rel_err  # noqa: E402
from relevance_factorizationmachine_amd import _lib, features, synth  # noqa: E402

K = 9
PAIRS_PER_BLOCK = 8_000_000
A_BLOCKS = 2
SHAPES = (("kuairec_small", 1411, 3327), ("kuairec_big", 7176, 10728))
FACTORS = (32, 400)


def tables(rng, nu, ni):
    user = np.hstack([np.eye(s)[rng.integers(0, s, size=nu)] for s in synth.KUAIREC_USER_GROUPS])
    item = np.hstack([rng.standard_normal((ni, 4)),
                      np.eye(synth.KUAIREC_N_TAGS)[rng.integers(0, synth.KUAIREC_N_TAGS, size=ni)]])
    return sp.csr_matrix(user), sp.csr_matrix(item), sp.csr_matrix(rng.standard_normal((nu, 1)))


def path_a_block(model, rt, users, nu, ni, ctx, user, item, keep_scores=False):
    """Top-K items of the users of one block through the pairs' design matrix."""
    import torch

    uu, ii = np.repeat(users, ni), np.tile(np.arange(ni), len(users))
    X = features.fm_features_kuairec(rt, uu, ii, nu, ni, features.take_rows(rt, ctx, uu), user, item)
    n = X.shape[0]
    scores = rt.empty((n,), torch.float64)
    _lib.check(rt.lib.rfm_fm_forward(rt.ctx, X.indptr.data_ptr(), X.indices.data_ptr(), X.values.data_ptr(), None, n,
                                     model.w0.dev.data_ptr(), model.w.dev.data_ptr(), model.V.dev.data_ptr(),
                                     model.n_features, model.n_factors, scores.data_ptr()))
    seg = rt.upload(np.arange(0, n + 1, ni, dtype=np.int32))
    labels = torch.ones((n,), dtype=torch.float64, device=rt.torch_device)
    pos = rt.empty((len(users), K), torch.int32)
    flags = rt.empty((len(users),), torch.int32)
    _lib.check(rt.lib.rfm_topk_users(rt.ctx, scores.data_ptr(), seg.data_ptr(), None, labels.data_ptr(), None, None,
                                     len(users), K, pos.data_ptr(), flags.data_ptr()))
    rt.sync()
    top = pos.cpu().numpy() - (np.arange(len(users), dtype=np.int32) * ni)[:, None]
    return top, (scores.cpu().numpy().reshape(len(users), ni) if keep_scores else None)


def clock(fn, rt, repeats):
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


def show(label, ms, scale=1.0, note=""):
    ms = ms * scale
    print(f"  {label}: {np.median(ms):10.2f} ms (min {ms.min():.2f}, max {ms.max():.2f}, {len(ms)} runs){note}", flush=True)
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only-b", action="store_true")
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import relevance_factorizationmachine_amd as pkg

    for name, nu, ni in SHAPES:
        user, item, ctx = tables(np.random.default_rng(1), nu, ni)
        per_block = max(1, PAIRS_PER_BLOCK // ni)
        blocks = [np.arange(b, min(b + per_block, nu)) for b in range(0, nu, per_block)]
        for k in FACTORS:
            model = pkg.FactorizationMachines(estimator="IPS", n_epochs=1, n_factors=k, lr=1e-4, batch_size=1, seed=7,
                                              n_features=synth.n_features_of(synth.SHAPES[name]), alpha=0.25)
            rt = model._rt
            sides = features.sides_kuairec(rt, nu, ni, ctx, user, item)
            print(f"{name} {nu} x {ni}, FM k = {k}, K = {K}", flush=True)
            b_ms = show("B recommend()", clock(lambda: model.recommend(sides, k=K), rt, args.repeats))
            if args.only_b:
                continue
            timed = blocks[:A_BLOCKS] if len(blocks) > A_BLOCKS else blocks
            scale = nu / sum(len(b) for b in timed)
            a_ms = show("A pairs' matrix -> forward -> rfm_topk_users",
                        clock(lambda: [path_a_block(model, rt, b, nu, ni, ctx, user, item) for b in timed], rt,
                              max(2, args.repeats // 2)), scale,
                        f" [extrapolated from {len(timed)} of {len(blocks)} user blocks]" if scale > 1 else "")
            print(f"  A / B = {a_ms / b_ms:.1f}", flush=True)
            top_a, scores_a = path_a_block(model, rt, blocks[0], nu, ni, ctx, user, item, keep_scores=True)
            scores_b = model.score_pairs(sides, users=blocks[0])
            err = rel_err(scores_b, scores_a)
            assert err < 1e-9, err
            assert_elementwise(scores_b, scores_a, what="score_pairs vs forward of the pairs' rows")
            top_b = model.recommend(sides, k=K, users=blocks[0])[0]
            print(f"  first block: probabilities rel_err {err:.2e}; top-{K} lists identical for "
                  f"{int((top_a == top_b).all(axis=1).sum())} of {len(blocks[0])} users", flush=True)
        # MF at k = 400: P, Q as they are initialised, b as fit() would set it
        mf = pkg.LogisticMatrixFactorization(estimator="IPS", n_epochs=1, n_factors=400, n_users=nu, n_items=ni, lr=0.02,
                                             reg=0.5, batch_size=1, seed=7)
        mf.b = 0.5
        print(f"{name} {nu} x {ni}, MF k = 400, K = {K}", flush=True)
        show("B recommend()", clock(lambda: mf.recommend(k=K), mf._rt, args.repeats))


if __name__ == "__main__":
    main()
