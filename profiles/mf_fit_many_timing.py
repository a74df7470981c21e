"""Timing of several MF models on one schedule on one GPU: what
profiles/n18/mf_fit_many_timing.txt records.

The KuaiRec-shaped MF configuration of bench.py's ``extra.mf``: the ``kuairec_small`` log, IPS,
lr = 0.01, reg = 0.5, B = 2 000, k = 400 and k = 16, 60 iterations; M models that differ in their seed.

  --mode fit    M calls of ``fit()`` one after the other (the baseline; run it on the PARENT commit's
                tree with ``--tree``: it uses nothing this commit adds);
  --mode many   one ``mf.fit_many`` of the same M models.

Per (k, M): one fit that is discarded, then ``--repeats`` timed ones; wall per call, per iteration and
per iteration and model.  Each mode writes a JSON file (``--json``); ``--report FIT.json MANY.json``
puts both tables and their ratio into ``--out``.  ``--cprofile`` (mode many) adds where the host side
of the largest M spends its time.

    python profiles/mf_fit_many_timing.py --mode fit --tree <parent tree> --json fit.json
    python profiles/mf_fit_many_timing.py --mode many --json many.json
    python profiles/mf_fit_many_timing.py --report fit.json many.json --out profiles/n18/mf_fit_many_timing.txt

The GPU time of rfm_mf_sgd_levels_many per level comes from a run of its own under
``rocprofv3 --kernel-trace --stats`` (``--mode many --models 16 --repeats 1``): the sequential
kernel's total time over the levels the JSON file counts."""
import argparse
import json
import os
import sys
import time

import numpy as np

ITERS, BATCH, LR, REG, SEED = 60, 2000, 0.01, 0.5, 12345


def levels_per_iteration(synth, runtime, train, shape, iters):
    ids = runtime.sample_batches(int(train["features"].shape[0]), BATCH, 0, iters)
    u, i = train["features"][:, 0], train["features"][:, 1]
    return [len(runtime.mf_schedule(u[r], i[r], shape.n_users, shape.n_items)[1]) - 1 for r in ids]


def measure(args):
    sys.path.insert(0, os.path.abspath(args.tree))
    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import mf, runtime, synth

    shape = synth.SHAPES["kuairec_small"]
    train, val = synth.make_log(shape, "MF", "IPS", seed=0, n_val=min(shape.n_val, 20000))
    levels = levels_per_iteration(synth, runtime, train, shape, args.iters)
    out = {"mode": args.mode, "package": os.path.dirname(pkg.__file__), "iters": args.iters,
           "levels_per_iteration": float(np.mean(levels)), "rows": []}

    def models(k, n):
        return [pkg.LogisticMatrixFactorization(estimator="IPS", n_epochs=args.iters, n_factors=k, n_users=shape.n_users,
                                                n_items=shape.n_items, lr=LR, reg=REG, batch_size=BATCH, seed=SEED + m)
                for m in range(n)]

    def run(ms):
        t0 = time.perf_counter()
        if args.mode == "fit":
            for m in ms:
                m.fit(train, val)
        else:
            mf.fit_many(ms, train, val)
        return time.perf_counter() - t0

    for k in args.ks:
        for n in args.models:
            run(models(k, n))  # discarded
            walls = [run(models(k, n)) for _ in range(args.repeats)]
            out["rows"].append({"k": k, "models": n, "wall_s": walls})
            print(k, n, ["%.4f" % w for w in walls], flush=True)
    if args.cprofile and args.mode == "many":
        import cProfile
        import io
        import pstats
        ms = models(args.ks[0], max(args.models))
        pr = cProfile.Profile()
        pr.enable()
        mf.fit_many(ms, train, val)
        pr.disable()
        buf = io.StringIO()
        pstats.Stats(pr, stream=buf).sort_stats("cumulative").print_stats(14)
        out["cprofile"] = {"k": args.ks[0], "models": max(args.models), "text": buf.getvalue()}
    with open(args.json, "w") as f:
        json.dump(out, f)


def report(fit_path, many_path, out_path):
    fit, many = json.load(open(fit_path)), json.load(open(many_path))
    iters = fit["iters"]
    assert iters == many["iters"]
    rows = {(r["k"], r["models"]): r["wall_s"] for r in many["rows"]}
    lines = [f"MF, kuairec_small log, IPS, lr {LR}, reg {REG}, B = {BATCH}, {iters} iterations, "
             f"{fit['levels_per_iteration']:.0f} levels per iteration (mean); models differ in their seed.",
             "Wall time of one call in ms: median of the timed repeats (all of them in brackets), the first call discarded.",
             "baseline: M calls of fit() in sequence (--mode fit; the tree it ran on is in its JSON file)",
             "fit_many: one call (--mode many)", "",
             "    k    M | M x fit(): ms   per iteration and model us | fit_many: ms   per iteration us   per iteration and model us | ratio"]
    for r in fit["rows"]:
        key = (r["k"], r["models"])
        if key not in rows:
            continue
        a, b = np.asarray(r["wall_s"]) * 1e3, np.asarray(rows[key]) * 1e3
        ma, mb, n = float(np.median(a)), float(np.median(b)), r["models"]
        br = lambda v: "/".join("%.1f" % x for x in v)  # noqa: E731
        lines.append(f"{r['k']:5d} {n:4d} | {ma:9.1f} ({br(a)})  {1e3 * ma / (iters * n):8.1f} | {mb:9.1f} ({br(b)})  "
                     f"{1e3 * mb / iters:8.1f}  {1e3 * mb / (iters * n):8.1f} | {ma / mb:6.2f}")
    if "cprofile" in many:
        c = many["cprofile"]
        lines += ["", f"host side of fit_many at k = {c['k']}, M = {c['models']} (cProfile, cumulative):", c["text"]]
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("\n".join(lines))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("fit", "many"))
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--json")
    ap.add_argument("--models", type=lambda s: [int(v) for v in s.split(",")], default=[1, 4, 16, 64])
    ap.add_argument("--ks", type=lambda s: [int(v) for v in s.split(",")], default=[400, 16])
    ap.add_argument("--iters", type=int, default=ITERS)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--cprofile", action="store_true")
    ap.add_argument("--report", nargs=2, metavar=("FIT.json", "MANY.json"))
    ap.add_argument("--out")
    args = ap.parse_args()
    if args.report:
        report(*args.report, args.out)
    else:
        measure(args)
