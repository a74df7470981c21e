#!/usr/bin/env python3
"""Per-iteration time of ``fit()`` with the catalogue metrics inside it, the forms
alternating in one process:

  N  no evaluator;
  V  the reference's ``ValEvaluator`` (IPS-DCG@5 over the rows of the validation log) computed on
     the device (``rfm_fm_train_eval`` / ``rfm_val_dcg``);
  C  ``evaluate.CatalogueValEvaluator`` with ``every = 1`` and ``every = 10``: side sums, the two
     rank passes and ``rfm_rank_metrics`` enqueued behind the iterations;

and, alone, one evaluation two ways: ``CatalogueValEvaluator.evaluate(model)`` and
``CatalogueEvaluator.evaluate(model)`` -- rank passes, download, host metrics, the only catalogue
evaluation there was before (this part also runs on a tree without the new class: ``--one-shot-only``).
The kernels of an evaluation are read from the trace (profiles/catalogue_val_prof.sh).

Shapes 1 411 x 3 327 and 7 176 x 10 728 (the synthetic KuaiRec-shaped logs, B = 2 000), FM k = 32 and
k = 400, MF k = 400; 10 and 100 held-out positives per user.  Device-synchronised host clock around
a whole ``fit()`` of ``--iters`` iterations after one warm-up fit, ``--repeats`` fits per form,
median / min / max of the per-iteration time.

usage (GPU box): python tests/manual/catalogue_val_timing.py [--shapes kuairec_small,kuairec_big]
    [--models fm32,fm400,mf400] [--positives 10,100] [--iters 300] [--repeats 3] [--one-shot-only]
    [--trace]
``--trace``: per configuration two fits of 20 iterations with the catalogue metrics after every
iteration and nothing else, the run to put under ``rocprofv3 --kernel-trace --memory-copy-trace
--hip-trace`` (profiles/catalogue_val_prof.sh)."""
import argparse
import os
import sys
import time

import numpy as np
from scipy import sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from relevance_factorizationmachine_amd import evaluate, features, synth  # noqa: E402

SIZES = {"kuairec_small": (1411, 3327), "kuairec_big": (7176, 10728)}
K_LIST, METRICS = [1, 5, 10, 100], ["DCG", "Recall", "MAP", "MRR", "AUC"]
HAVE_NEW = hasattr(evaluate, "CatalogueValEvaluator")
TRACE_ITERS = 20  # iterations of a --trace fit (profiles/catalogue_val_trace_summary.py --iters)


class ValEvaluatorLike:
    """The attributes of the reference's ValEvaluator (utils/evaluate.py:22-33,160-207); opts in to
    the device metric."""

    metric_name, k, rfm_device_evaluator = "DCG", 5, True

    def __init__(self, frame, feats):
        self.interaction_df, self.features = frame, feats


def tables(rng, nu, ni):
    user = np.hstack([np.eye(s)[rng.integers(0, s, size=nu)] for s in synth.KUAIREC_USER_GROUPS])
    item = np.hstack([rng.standard_normal((ni, 4)),
                      np.eye(synth.KUAIREC_N_TAGS)[rng.integers(0, synth.KUAIREC_N_TAGS, size=ni)]])
    return sp.csr_matrix(user), sp.csr_matrix(item), sp.csr_matrix(rng.standard_normal((nu, 1)))


def heldout(rng, nu, ni, per_user, train_pairs):
    """``per_user`` distinct items per user that are not train pairs, and the train pairs as exclusion lists."""
    E = sp.csr_matrix((np.ones(train_pairs.shape[0]), (train_pairs[:, 0], train_pairs[:, 1])), shape=(nu, ni))
    E.sum_duplicates()
    users = np.repeat(np.arange(nu), per_user)
    items = np.concatenate([rng.choice(ni, size=per_user, replace=False) for _ in range(nu)])
    keep = np.asarray(E[users, items]).ravel() == 0
    return (users[keep], items[keep]), E


def stats(label, per_iter_ms):
    a = np.asarray(per_iter_ms)
    print(f"  {label}: {np.median(a):9.4f} ms/iteration (min {a.min():.4f}, max {a.max():.4f}, {len(a)} fits)", flush=True)


def clock(fn, rt, repeats):
    fn()
    out = []
    for _ in range(repeats):
        rt.sync()
        t0 = time.perf_counter()
        fn()
        rt.sync()
        out.append(1e3 * (time.perf_counter() - t0))
    return np.asarray(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="kuairec_small,kuairec_big")
    ap.add_argument("--models", default="fm32,fm400,mf400")
    ap.add_argument("--positives", default="10,100")
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--one-shot-only", action="store_true")
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import relevance_factorizationmachine_amd as pkg

    print(f"CatalogueValEvaluator present: {HAVE_NEW}", flush=True)
    iters = TRACE_ITERS if args.trace else args.iters
    for name in args.shapes.split(","):
        nu, ni = SIZES[name]
        rng = np.random.default_rng(1)
        user, item, ctx = tables(rng, nu, ni)
        logs = {kind: synth.make_log(name, kind, "IPS", seed=0) for kind in ("FM", "MF")}
        pairs_val = logs["MF"][1]["features"]
        frame = synth.interaction_frame(logs["MF"][1], pairs_val)
        for which in args.models.split(","):
            kind, k = which[:2].upper(), int(which[2:])
            train, val = logs[kind]
            for per_user in (int(v) for v in args.positives.split(",")):
                positives, E = heldout(np.random.default_rng(per_user), nu, ni, per_user, logs["MF"][0]["features"])
                print(f"{name} {nu} x {ni}, {kind} k = {k}, {per_user} held-out positives per user "
                      f"({positives[0].shape[0]} in all), B = {synth.SHAPES[name].batch_size}, {iters} iterations", flush=True)

                def model(evaluator=None, n_epochs=iters):
                    common = dict(estimator="IPS", n_epochs=n_epochs, n_factors=k, batch_size=synth.SHAPES[name].batch_size,
                                  seed=7, evaluator=evaluator)
                    if kind == "FM":
                        return pkg.FactorizationMachines(n_features=synth.n_features_of(synth.SHAPES[name]), lr=1e-6,
                                                         alpha=0.25, **common)
                    return pkg.LogisticMatrixFactorization(n_users=nu, n_items=ni, lr=0.01, reg=0.5, **common)

                rt = model(n_epochs=1)._rt
                sides = features.sides_kuairec(rt, nu, ni, ctx, user, item) if kind == "FM" else None

                def catalogue(every):
                    return evaluate.CatalogueValEvaluator(positives, ni, K_LIST, METRICS, ("DCG", 5), sides=sides,
                                                          exclude=E, every=every)

                forms = [("N no evaluator", lambda: None),
                         ("V ValEvaluator on the device", lambda: ValEvaluatorLike(frame, {kind: val["features"]}))]
                if HAVE_NEW:
                    forms += [("C catalogue metrics, every = 1", lambda: catalogue(1)),
                              ("C catalogue metrics, every = 10", lambda: catalogue(10))]
                if args.trace:  # runs of exactly `iters` evaluations: what the summary cuts the trace by
                    forms = [f for f in forms if f[0].endswith("every = 1")]
                if not args.one_shot_only:
                    evaluators = [(label, make()) for label, make in forms]  # (uploaded once, as a search would)
                    times = {label: [] for label, _ in forms}
                    for label, ev in evaluators:  # warm-up: uploads, plans, allocator pools
                        model(ev, n_epochs=min(iters, 20)).fit(train, val)
                    for _ in range(1 if args.trace else args.repeats):  # alternating: drift hits every form alike
                        for label, ev in evaluators:
                            m = model(ev)
                            rt.sync()
                            t0 = time.perf_counter()
                            m.fit(train, val)
                            rt.sync()
                            times[label].append(1e3 * (time.perf_counter() - t0) / iters)
                    for label, _ in forms:
                        stats(label, times[label])
                if args.trace:
                    continue
                # one evaluation, alone
                m = model(n_epochs=2)
                m.fit(train, val)
                old = evaluate.CatalogueEvaluator(positives, ni, K_LIST, METRICS, exclude=E)
                ms = clock(lambda: old.evaluate(m, sides), rt, max(args.repeats, 3))
                print(f"  one CatalogueEvaluator.evaluate(model) (rank passes, download, host metrics): "
                      f"{np.median(ms):9.2f} ms (min {ms.min():.2f}, max {ms.max():.2f})", flush=True)
                if HAVE_NEW:
                    ev = catalogue(1)
                    ms = clock(lambda: ev.evaluate(m), rt, max(args.repeats, 3))
                    print(f"  one CatalogueValEvaluator.evaluate(model) (all on the device):            "
                          f"{np.median(ms):9.2f} ms (min {ms.min():.2f}, max {ms.max():.2f})", flush=True)


if __name__ == "__main__":
    main()
