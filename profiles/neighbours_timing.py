"""Whole-call timing of ``similar_items`` over all items on one GPU: what
profiles/n27/neighbours_timing.txt records.

Catalogues of 10 728 items (KuaiRec big) and 3 327 (small), k = 32 and 400, K = 9, cosine, MF (rows
of Q) and FM (b_i of an item side of one-hot id + 4 dense + 31 tag columns).  Per case, host clock
around the call, synchronised before and after, median and range of ``--repeats`` calls after a
warm-up call:

  similar_items  the model method: (FM: one side-sum launch,) rfm_rows_normalise, rfm_pair_topk_raw,
                 the lists copied to the host
  torch          the only path a user had for the same answer before: the same vectors (FM: from
                 the same side-sum launch) normalised with torch, a float64 B^ B^T, the diagonal
                 set to -inf, torch.topk, the lists copied to the host
  side sums / normalise / tile
                 the three stages of similar_items alone, each synchronised by itself (the tile:
                 both launches of rfm_pair_topk_raw with the self-exclusion lists already uploaded)

    python profiles/neighbours_timing.py --out profiles/n27/neighbours_timing.txt

The file is this script's output and nothing else: a run overwrites it."""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CATALOGUES = (10728, 3327)
FACTORS = (32, 400)
K = 9
N_USERS = 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()

    import scipy.sparse as sp
    import torch

    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import _lib
    from relevance_factorizationmachine_amd import recommend as rec
    from relevance_factorizationmachine_amd.runtime import Runtime

    rt = Runtime.get()
    lines = [f"similar_items over all items, K = {K}, cosine; us per call, median (smallest - largest) of "
             f"{args.repeats} calls after a warm-up call; {torch.cuda.get_device_name(0)}", ""]

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

    def torch_lists(B, kf):
        Bn = B[:, :kf] / torch.linalg.norm(B[:, :kf], dim=1, keepdim=True)
        S = Bn @ Bn.T
        S.fill_diagonal_(float("-inf"))
        values, ids = torch.topk(S, K, dim=1)
        return ids.cpu().numpy(), values.cpu().numpy()

    def tile_alone(R, kf):
        """The launches of rfm_pair_topk_raw as recommend.neighbours makes them, on rows normalised before."""
        n = int(R.shape[0])
        B = rec.normalised(rt, R, kf)[0]
        zero = torch.zeros((n,), dtype=torch.float64, device=rt.torch_device)
        ops = rec.Operands(rt, B, zero, B, zero, zero, kf)
        excl = rec._exclusions(rt, rec.check_neighbours(n, K)[2])
        ws = rt.empty((rec.topk_workspace_bytes(n, n, K),), torch.uint8)
        ids, values = rt.empty((n, K), torch.int32), rt.empty((n, K), torch.float64)
        return lambda: _lib.check(rt.lib.rfm_pair_topk_raw(*ops.pair_args(None, n), *rec.excl_args(excl), K,
                                                           ws.data_ptr(), ids.data_ptr(), values.data_ptr()))

    for n_items in CATALOGUES:
        for kf in FACTORS:
            rng = np.random.default_rng([n_items, kf])
            # MF
            mf = pkg.LogisticMatrixFactorization(estimator="IPS", n_epochs=1, n_factors=kf, n_users=N_USERS,
                                                 n_items=n_items, lr=0.02, reg=0.5, batch_size=1, seed=1)
            mf.P.set(rng.standard_normal((N_USERS, kf)))
            mf.Q.set(rng.standard_normal((n_items, kf)))
            mf.b_u.set(np.zeros(N_USERS))
            mf.b_i.set(np.zeros(n_items))
            mf.b = 0.0
            ids, values = mf.similar_items(K)
            t_ids, t_values = torch_lists(mf.Q.dev, kf)
            agree = float(np.mean(ids == t_ids))
            lines += [f"MF  n_items = {n_items}, k = {kf}   (lists equal to torch's at {100 * agree:.2f} % of the positions, "
                      f"largest |value - torch's| {np.max(np.abs(values - t_values)):.2e})",
                      f"  similar_items {timed(lambda: mf.similar_items(K))}",
                      f"  torch         {timed(lambda: torch_lists(mf.Q.dev, kf))}",
                      f"  normalise     {timed(lambda: rec.normalised(rt, mf.Q.dev, kf))}",
                      f"  tile          {timed(tile_alone(mf.Q.dev, kf))}", ""]
            # FM
            tags = sp.csr_matrix((rng.random((n_items, 31)) < 0.1).astype(np.float64))
            dense = sp.csr_matrix(rng.standard_normal((n_items, 4)))
            XI = sp.hstack([sp.csr_matrix((n_items, N_USERS)), sp.identity(n_items, format="csr"), dense, tags]).tocsr()
            XU = sp.hstack([sp.identity(N_USERS, format="csr"), sp.csr_matrix((N_USERS, n_items + 35))]).tocsr()
            sides = rec.Sides(XU, XI)
            fm = pkg.FactorizationMachines(estimator="IPS", n_epochs=1, n_factors=kf, n_features=sides.n_features,
                                           lr=1e-4, batch_size=1, seed=1)
            fm.w0.set(np.zeros(1))
            fm.w.set(rng.standard_normal(sides.n_features))
            fm.V.set(0.3 * rng.standard_normal((sides.n_features, kf)))
            X = sides.device(rt)[1]
            sums = lambda: rec.side_sums(rt, X, fm.w.dev, fm.V.dev, fm.n_features, kf)  # noqa: E731
            ids, values = fm.similar_items(sides, K)
            t_ids, t_values = torch_lists(sums()[0], kf)
            agree = float(np.mean(ids == t_ids))
            lines += [f"FM  n_items = {n_items}, k = {kf}, {XI.nnz / n_items:.1f} entries per item   (lists equal to torch's at "
                      f"{100 * agree:.2f} % of the positions, largest |value - torch's| {np.max(np.abs(values - t_values)):.2e})",
                      f"  similar_items {timed(lambda: fm.similar_items(sides, K))}",
                      f"  torch         {timed(lambda: torch_lists(sums()[0], kf))}",
                      f"  side sums     {timed(sums)}",
                      f"  normalise     {timed(lambda: rec.normalised(rt, sums()[0], kf))}   (with the side sums)",
                      f"  tile          {timed(tile_alone(sums()[0], kf))}", ""]
            del mf, fm, sides
            torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
