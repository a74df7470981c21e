"""Whole-call timing of ``recommend_users`` over every item on one GPU, against the
PARENT commit's ``recommend()`` on a synthetic catalogue with the two counts exchanged: what
profiles/n29/audience_timing.txt records.

The reference's KuaiRec catalogue shape, 10 728 items over 7 176 users, k = 400 factors, K = 9, FM
(both sides: one-hot id + 4 dense + 31 tag columns) and MF.  One process times one tree in one
direction; the two are run alternately, three rounds:

  --direction audience   this tree: recommend_users(K) for all 10 728 items, 7 176 users the candidates
  --direction forward    the tree under --tree (the parent's checkout with its own library):
                         recommend(K) for 10 728 USERS over 7 176 ITEMS -- the same two tables with
                         their roles exchanged, hence the same tiles, splits and merge launch

    python profiles/audience_timing.py --direction audience --label "round 1 this"
    RFM_LIB_PATH=PARENT/relevance_factorizationmachine_amd/librfm_hip.so \\
        python profiles/audience_timing.py --direction forward --tree PARENT --label "round 1 parent"

Per model one line: host clock around the call, synchronised before and after, the lists copied to
the host inside it; median (smallest - largest) of ``--repeats`` calls after a warm-up call, in us.
``--out`` appends the lines to a file."""
import argparse
import os
import sys
import time

import numpy as np

N_QUERIES, N_CANDIDATES, FACTORS, K = 10728, 7176, 400, 9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--direction", choices=("audience", "forward"), required=True)
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))

    import scipy.sparse as sp
    import torch

    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import recommend as rec
    from relevance_factorizationmachine_amd.runtime import Runtime

    rt = Runtime.get()
    audience = args.direction == "audience"
    kf = FACTORS
    rng = np.random.default_rng([N_QUERIES, N_CANDIDATES, kf])
    lines = []

    def timed(call):
        call()
        out = []
        for _ in range(args.repeats):
            rt.sync()
            torch.cuda.synchronize()
            t = time.perf_counter()
            call()
            rt.sync()
            torch.cuda.synchronize()
            out.append((time.perf_counter() - t) * 1e6)
        return f"{np.median(out):10.0f} ({min(out):.0f} - {max(out):.0f})"

    # the two tables by role: the queries' (10 728 rows) and the candidates' (7 176 rows).  In the
    # audience direction the queries are the items, in the forward one the users.
    Tq, Tc = rng.standard_normal((N_QUERIES, kf)) * kf ** -0.25, rng.standard_normal((N_CANDIDATES, kf)) * kf ** -0.25
    bq, bc = 0.5 * rng.standard_normal(N_QUERIES), 0.5 * rng.standard_normal(N_CANDIDATES)
    n_users, n_items = (N_CANDIDATES, N_QUERIES) if audience else (N_QUERIES, N_CANDIDATES)
    mf = pkg.LogisticMatrixFactorization(estimator="IPS", n_epochs=1, n_factors=kf, n_users=n_users, n_items=n_items,
                                         lr=0.02, reg=0.5, batch_size=1, seed=1)
    for handle, value in zip((mf.P, mf.b_u, mf.Q, mf.b_i), (Tc, bc, Tq, bq) if audience else (Tq, bq, Tc, bc)):
        handle.set(value)
    mf.b = 0.37
    call = (lambda: mf.recommend_users(K)) if audience else (lambda: mf.recommend(K))
    ids, _ = call()
    assert ids.shape == (N_QUERIES, K) and (ids >= 0).all()
    lines.append(f"{args.label:16} MF {'recommend_users' if audience else 'recommend      '} {timed(call)}")

    def side(n):
        extra = sp.hstack([sp.csr_matrix(rng.standard_normal((n, 4))),
                           sp.csr_matrix((rng.random((n, 31)) < 0.1).astype(np.float64))])
        return sp.identity(n, format="csr"), extra

    idq, xq = side(N_QUERIES)
    idc, xc = side(N_CANDIDATES)
    pad = sp.csr_matrix
    # columns: [query ids | candidate ids | 35 query columns | 35 candidate columns]
    Xq = sp.hstack([idq, pad((N_QUERIES, N_CANDIDATES)), xq, pad((N_QUERIES, 35))]).tocsr()
    Xc = sp.hstack([pad((N_CANDIDATES, N_QUERIES)), idc, pad((N_CANDIDATES, 35)), xc]).tocsr()
    sides = rec.Sides(Xc, Xq) if audience else rec.Sides(Xq, Xc)
    fm = pkg.FactorizationMachines(estimator="IPS", n_epochs=1, n_factors=kf, n_features=sides.n_features, lr=1e-4,
                                   batch_size=1, seed=1)
    fm.w0.set(np.array([0.37]))
    fm.w.set(0.1 * rng.standard_normal(sides.n_features))
    fm.V.set(0.1 * rng.standard_normal((sides.n_features, kf)))
    call = (lambda: fm.recommend_users(sides, K)) if audience else (lambda: fm.recommend(sides, K))
    ids, _ = call()
    assert ids.shape == (N_QUERIES, K) and (ids >= 0).all()
    lines.append(f"{args.label:16} FM {'recommend_users' if audience else 'recommend      '} {timed(call)}"
                 f"   ({Xq.nnz / N_QUERIES:.1f} and {Xc.nnz / N_CANDIDATES:.1f} entries per row)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
