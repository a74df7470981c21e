"""Whole-call timing of fold-in with the examples grouped on the host and on the device
on one GPU: what profiles/n19/fold_group_timing.txt records.

The cases are N13's a. for MF and N16's a. for FM: 10 728 items, 7 176 new users whose example counts are
log-normal (median 61, clipped at 5 000: about a million examples, shuffled), at k = 32 and k = 400, one
pass.  Per model and k, the wall time of one ``fold_in_users`` call (synchronised before and after):

  host      the log in NumPy, grouped by ``fold.fold_examples`` on the host (``group=None``): the only path of
            the parent commit, and this tree's default for a host log
  device    the same NumPy log, uploaded as it is and grouped by ``rfm_fold_group`` (``group="device"``)
  resident  the log already on the device as tensors (``group=None``), with ``check=True`` (one wait for
            the status words) and with ``check=False``

and the grouping launches alone (events around ``rfm_fold_group`` on the resident log), also for two
worst cases of the same size: one row holding every example (the walk of a bin beyond the LDS cap), and
every row holding one example (all rows in one bin of the order pass).

``--parent DIR`` names a checkout of the parent commit with its own build; the baseline rows are measured
there, in a process of its own, alternating with this tree's: parent, this, parent, this, ...  Without it
the host rows of this tree stand in (the host path's code is the parent's).  Every figure is a median of
``--repeats`` calls after a warm-up call; the spread is the largest minus the smallest over all runs of a
row.

    python profiles/fold_group_timing.py --out profiles/n19/fold_group_timing.txt --parent ../parent

The file is this script's output and nothing else: a run overwrites it."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

N_ITEMS, N_NEW, N_OLD, UW, IW = 10728, 7176, 8, 16, 16
LR = 1e-5
KS = (32, 400)


def case_a():
    rng = np.random.default_rng(13)
    lengths = np.clip(rng.lognormal(np.log(60.0), 1.3, size=N_NEW).astype(np.int64), 1, 5000)
    n_ex = int(lengths.sum())
    users = np.repeat(np.arange(N_NEW), lengths)
    data = {"features": np.stack([users, rng.integers(0, N_ITEMS, size=n_ex)], axis=1)[rng.permutation(n_ex)],
            "labels": (rng.random(n_ex) < 0.5).astype(np.float64), "pscores": rng.uniform(0.1, 1.0, size=n_ex) ** 0.5}
    return data, lengths


def worker(tree, out_path, repeats):
    """One tree's rows, as JSON: {row: [us of each repeat]}."""
    sys.path.insert(0, tree)
    import scipy.sparse as sp
    import torch

    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import fold
    from relevance_factorizationmachine_amd import recommend as rec

    has_group = hasattr(fold, "group_examples_device")
    data, lengths = case_a()
    n_ex = len(data["labels"])
    rng = np.random.default_rng(7)
    rows = {}

    def timed(call, rt):
        call()
        out = []
        for _ in range(repeats):
            rt.sync()
            t = time.perf_counter()
            call()
            rt.sync()
            out.append((time.perf_counter() - t) * 1e6)
        return out

    def modes(rt, fold_in):
        m = {"host": lambda: fold_in(data)}
        if has_group:
            dev = {k: rt.upload(v) for k, v in data.items()}
            m["device"] = lambda: fold_in(data, group="device")
            m["resident"] = lambda: fold_in(dev)
            m["resident check=False"] = lambda: fold_in(dev, check=False)
        return m

    def table(n, width):
        T = (rng.random((n, width)) < 0.3).astype(np.float64)
        T[:, 0] = 1.0
        return sp.csr_matrix(T)

    n_features = N_OLD + UW + N_ITEMS + IW
    XU = sp.hstack([sp.identity(N_OLD), table(N_OLD, UW), sp.csr_matrix((N_OLD, N_ITEMS + IW))]).tocsr()
    XI = sp.hstack([sp.csr_matrix((N_ITEMS, N_OLD + UW)), sp.identity(N_ITEMS), table(N_ITEMS, IW)]).tocsr()
    new_rows = sp.hstack([sp.csr_matrix((N_NEW, N_OLD)), table(N_NEW, UW), sp.csr_matrix((N_NEW, N_ITEMS + IW))]).tocsr()
    sides = rec.Sides(XU, XI)
    rt = None
    for k in KS:
        mf = pkg.LogisticMatrixFactorization(estimator="IPS", n_epochs=1, n_factors=k, lr=0.01, batch_size=1000, seed=1,
                                             n_users=N_OLD, n_items=N_ITEMS, reg=1e-4)
        mf.b = 0.1
        rt = mf._rt
        for name, call in modes(rt, lambda d, **kw: mf.fold_in_users(d, N_NEW, 1, **kw)).items():
            rows[f"mf k={k} {name}"] = timed(call, rt)
        fm = pkg.FactorizationMachines(estimator="IPS", n_epochs=1, n_factors=k, lr=LR, batch_size=1000, seed=1,
                                       n_features=n_features, alpha=0.3)
        for name, call in modes(rt, lambda d, **kw: fm.fold_in_users(sides, new_rows, d, 1, **kw)).items():
            rows[f"fm k={k} {name}"] = timed(call, rt)
    if has_group:
        one_row = {**data, "features": np.stack([np.zeros(n_ex, np.int64), data["features"][:, 1]], axis=1)}
        singles = {**data, "features": np.stack([rng.permutation(n_ex), data["features"][:, 1]], axis=1)}
        for name, d, n_new in (("case a", data, N_NEW), ("one row holds every example", one_row, N_NEW),
                               ("every row holds one example", singles, n_ex)):
            dev = {k: rt.upload(v) for k, v in d.items()}

            def launches():
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                fold.group_examples_device(rt, dev, n_new, N_ITEMS, 0, check=False)
                t1.record()
                t1.synchronize()
                return t0.elapsed_time(t1) * 1e3
            launches()
            rows[f"grouping launches alone, {name}"] = [launches() for _ in range(repeats)]
            if name != "case a":
                mf32 = pkg.LogisticMatrixFactorization(estimator="IPS", n_epochs=1, n_factors=32, lr=0.01, batch_size=1000,
                                                       seed=1, n_users=N_OLD, n_items=N_ITEMS, reg=1e-4)
                mf32.b = 0.1
                rows[f"mf k=32 {name}: host"] = timed(lambda: mf32.fold_in_users(d, n_new, 1), rt)
                rows[f"mf k=32 {name}: resident"] = timed(lambda: mf32.fold_in_users(dev, n_new, 1), rt)
    meta = {"device": torch.cuda.get_device_name(0), "n_ex": n_ex, "median": int(np.median(lengths)),
            "longest": int(lengths.max())}
    with open(out_path, "w") as f:
        json.dump({"meta": meta, "rows": rows}, f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--parent", help="a checkout of the parent commit, built")
    ap.add_argument("--pairs", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--worker", nargs=2, metavar=("TREE", "JSON"))
    args = ap.parse_args()
    if args.worker:
        return worker(os.path.abspath(args.worker[0]), args.worker[1], args.repeats)
    here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out_dir = os.path.dirname(os.path.abspath(args.out))
    os.makedirs(out_dir, exist_ok=True)
    trees = ([("parent", os.path.abspath(args.parent))] if args.parent else []) + [("this", here)]
    runs = {name: [] for name, _ in trees}
    for i in range(args.pairs):
        for name, tree in trees:
            path = os.path.join(out_dir, f".fold_group_{name}_{i}.json")
            env = {k: v for k, v in os.environ.items() if k != "RFM_LIB_PATH"}
            subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", tree, path, "--repeats", str(args.repeats)],
                           check=True, cwd=tree, env=env, timeout=600)
            runs[name].append(json.load(open(path)))
            os.remove(path)
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    def stats(name, row):
        v = [u for r in runs[name] for u in r["rows"].get(row, [])]
        return (float(np.median(v)), max(v) - min(v), len(v)) if v else None

    meta = runs["this"][0]["meta"]
    say(f"device {meta['device']}")
    say(f"{N_NEW} new users, {N_ITEMS} items, {meta['n_ex']} examples, example counts median {meta['median']}, longest "
        f"{meta['longest']}; one pass; ms, median (spread = largest - smallest) over {args.pairs} processes a tree x "
        f"{args.repeats} calls, run in the order " + ", ".join(n for n, _ in trees) + ", ...")
    base = "parent" if args.parent else "this"
    say(f"baseline: the host path of {'the parent commit' if args.parent else 'this tree (no --parent given)'}")
    say()
    say(f"{'row':<44}{'median':>10}{'spread':>10}   against the baseline")
    verdicts = []
    for model in ("mf", "fm"):
        for k in KS:
            b = stats(base, f"{model} k={k} host")
            say(f"{model + ' k=' + str(k) + ' host (' + base + ')':<44}{b[0] / 1e3:>10.2f}{b[1] / 1e3:>10.2f}")
            for mode in (["host"] if args.parent else []) + ["device", "resident", "resident check=False"]:
                s = stats("this", f"{model} k={k} {mode}")
                holds = b[0] - s[0] > b[1] + s[1]
                say(f"{model + ' k=' + str(k) + ' ' + mode + ' (this)':<44}{s[0] / 1e3:>10.2f}{s[1] / 1e3:>10.2f}   "
                    f"{b[0] / s[0]:.2f}x; shorter by more than both spreads: {'yes' if holds else 'no'}")
                if mode == "resident":
                    verdicts.append((f"{model} k={k}", holds))
    say()
    for name in ("case a", "one row holds every example", "every row holds one example"):
        s = stats("this", f"grouping launches alone, {name}")
        say(f"{'grouping launches alone, ' + name:<56}{s[0] / 1e3:>10.3f}{s[1] / 1e3:>10.3f}")
        if name != "case a":
            for mode in ("host", "resident"):
                s = stats("this", f"mf k=32 {name}: {mode}")
                say(f"{'  mf k=32 whole call, ' + mode + ' (this)':<56}{s[0] / 1e3:>10.2f}{s[1] / 1e3:>10.2f}")
    say()
    say("The device-resident call is shorter than the baseline by more than the two spreads together: "
        + ", ".join(f"{n}: {'yes' if h else 'NO'}" for n, h in verdicts) + ".")
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
