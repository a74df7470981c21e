"""Timing of ``recommend_diverse`` on one GPU: what profiles/n30/diverse_timing.txt records.

The reference's KuaiRec catalogue shape, all 7 176 users over 10 728 items, depth 256, k = 9, trade_off
0.5, cosine; 32 and 400 factors; MF and FM (both sides: one-hot id + 4 dense + 31 tag columns).  Host
clock around each call, synchronised before and after, median (smallest - largest) of ``--repeats``
calls after a warm-up call, in us, ``--rounds`` rounds.  Per model and factor count:

  whole call      recommend_diverse(9, 256, 0.5): ranking, normalisation, selection, the lists on the host
  rank_catalogue  rank_catalogue(256) alone on the same users, its lists on the host
  ranking         the split of the whole call: rank_catalogue_device, left on the device
  normalisation   rfm_rows_normalise of the item table
  selection       the one rfm_diverse_select launch on those candidates, synchronised
  torch           the only path a user had before: the same greedy rule in torch float64 on the same
                  device from the same device ranking and rows, in user blocks whose
                  [block, 256, factors] gather fits, a host loop over k; its lists on the host

The torch lists must equal the kernel's at every position (asserted).  The selection's byte model is
k * depth * kpad * 8 bytes of rows per user; the rate reached is set against the gather rates of the
table's size class measured on this device family: rows of a table that fits an XCD's L2 (the 2.7 MB
table at 32 factors) 16.8 TB/s, uniformly random rows of a 38 MB table (34 MB at 400 factors) from
the Infinity Cache 8.6 TB/s.  ``--out`` appends the lines to a file."""
import argparse
import os
import sys
import time

import numpy as np

N_USERS, N_ITEMS, DEPTH, K, TRADE_OFF = 7176, 10728, 256, 9, 0.5
GATHER_TBS = {32: 16.8, 400: 8.6}


def torch_mmr(torch, cand_items, cand_scores, R, kf, k, lam, block):
    """Greedy MMR in torch float64: ``(items [n, k])`` on the host."""
    n, depth = cand_items.shape
    out = torch.empty((n, k), dtype=torch.int64, device=cand_items.device)
    rows_of = torch.arange(block, device=cand_items.device)
    for lo in range(0, n, block):
        it = cand_items[lo:lo + block].long()
        b = it.shape[0]
        rows = R[:, :kf][it]                                # [b, depth, kf]
        base = lam * cand_scores[lo:lo + block]
        m = torch.full((b, depth), -float("inf"), dtype=torch.float64, device=it.device)
        taken = torch.zeros((b, depth), dtype=torch.bool, device=it.device)
        for t in range(k):
            v = base if t == 0 else base - (1.0 - lam) * m
            pick = torch.where(taken, -float("inf"), v).argmax(dim=1)
            out[lo:lo + b, t] = it[rows_of[:b], pick]
            taken[rows_of[:b], pick] = True
            if t + 1 < k:
                s = torch.einsum("bdf,bf->bd", rows, rows[rows_of[:b], pick])
                m = torch.maximum(m, torch.nan_to_num(s, nan=0.0))
    return out.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--factors", type=int, nargs="+", default=[32, 400])
    ap.add_argument("--repeats", type=int, default=7)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--block", type=int, default=1024)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

    import scipy.sparse as sp
    import torch

    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import recommend as rec
    from relevance_factorizationmachine_amd.runtime import Runtime

    rt = Runtime.get()
    lines = []

    def say(line):
        print(line, flush=True)
        lines.append(line)

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
        return float(np.median(out)), f"{np.median(out):10.0f} ({min(out):.0f} - {max(out):.0f})"

    def models(kf):
        rng = np.random.default_rng([N_USERS, N_ITEMS, kf])
        mf = pkg.LogisticMatrixFactorization(estimator="IPS", n_epochs=1, n_factors=kf, n_users=N_USERS, n_items=N_ITEMS,
                                             lr=0.02, reg=0.5, batch_size=1, seed=1)
        for handle, value in zip((mf.P, mf.b_u, mf.Q, mf.b_i),
                                 (rng.standard_normal((N_USERS, kf)) * kf ** -0.25, 0.5 * rng.standard_normal(N_USERS),
                                  rng.standard_normal((N_ITEMS, kf)) * kf ** -0.25, 0.5 * rng.standard_normal(N_ITEMS))):
            handle.set(value)
        mf.b = 0.37
        yield "MF", mf, None

        def side(n):
            return sp.identity(n, format="csr"), sp.hstack([sp.csr_matrix(rng.standard_normal((n, 4))),
                                                            sp.csr_matrix((rng.random((n, 31)) < 0.1).astype(np.float64))])

        (idu, xu), (idi, xi) = side(N_USERS), side(N_ITEMS)
        pad = sp.csr_matrix
        XU = sp.hstack([idu, pad((N_USERS, N_ITEMS)), xu, pad((N_USERS, 35))]).tocsr()
        XI = sp.hstack([pad((N_ITEMS, N_USERS)), idi, pad((N_ITEMS, 35)), xi]).tocsr()
        sides = rec.Sides(XU, XI)
        fm = pkg.FactorizationMachines(estimator="IPS", n_epochs=1, n_factors=kf, n_features=sides.n_features, lr=1e-4,
                                       batch_size=1, seed=1)
        fm.w0.set(np.array([0.37]))
        fm.w.set(0.1 * rng.standard_normal(sides.n_features))
        fm.V.set(0.1 * rng.standard_normal((sides.n_features, kf)))
        yield "FM", fm, sides

    for kf in args.factors:
        kpad = rec.pad4(kf)
        model_bytes = N_USERS * K * DEPTH * kpad * 8
        for name, model, sides in models(kf):
            lead = () if sides is None else (sides,)
            whole = lambda: model.recommend_diverse(*lead, K, DEPTH, TRADE_OFF)  # noqa: E731
            catalogue = lambda: model.rank_catalogue(*lead, DEPTH)  # noqa: E731
            ops = rec.operands(model, sides)
            ranking = lambda: rec.rank_catalogue_device(*ops, DEPTH)  # noqa: E731
            normalise = lambda: rec.normalised(rt, ops.B, kf)  # noqa: E731
            cand_items, cand_scores, _ = ranking()
            R = normalise()[0]
            select = lambda: rec.diversify(rt, cand_items, cand_scores, R, kf, K, TRADE_OFF)  # noqa: E731

            def torch_path():
                ci, cs, _ = rec.rank_catalogue_device(*ops, DEPTH)
                rows = rec.normalised(rt, ops.B, kf)[0]
                rt.sync()
                return torch_mmr(torch, ci, cs, rows, kf, K, TRADE_OFF, args.block)

            items = whole()[0]
            assert items.shape == (N_USERS, K) and (items >= 0).all()
            differ = int((torch_path() != items).sum())
            say(f"{name} {kf:3} factors: positions at which the torch lists differ from the kernel's: {differ} of {items.size}")
            assert differ == 0
            for r in range(args.rounds):
                for what, call in (("whole call", whole), ("rank_catalogue", catalogue), ("ranking", ranking),
                                   ("normalisation", normalise), ("selection", select), ("torch", torch_path)):
                    med, text = timed(call)
                    extra = ""
                    if what == "selection":
                        rate = model_bytes / (med * 1e-6) / 1e12
                        extra = (f"   byte model {model_bytes / 1e9:.2f} GB -> {rate:.2f} TB/s, "
                                 f"{100 * rate / GATHER_TBS.get(kf, 8.6):.0f} % of {GATHER_TBS.get(kf, 8.6)} TB/s")
                    say(f"round {r + 1} {name} {kf:3} factors {what:15} {text}{extra}")
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
