#!/usr/bin/env python3
"""What small fits leave behind -- parameters, both loss lists, ``val_metrics`` -- in one .npz, to
compare two trees of the HOST code (the fit drivers of fm.py, mf.py, dist.py, evaluate.py) bit for
bit on the same build of the library:

  fm_none, fm_device, fm_host, fm_catalogue   FactorizationMachines.fit, ``deterministic = True``, 19
                                              iterations (id chunks of 16 + 3): no evaluator; a
                                              ValEvaluator on the device, three iterations per chunk
                                              of score slots; the same as a host callback; a
                                              CatalogueValEvaluator every 5 iterations
  dp_rows, dp_dense                           dist.fit_data_parallel on one rank with the exchange
                                              forced (RFM_DP_FORCE_EXCHANGE=1), the device evaluator
  mf_exact                                    LogisticMatrixFactorization.fit (exact mode), the device
                                              evaluator, three iterations per chunk of score slots

Left out: MF HOGWILD, and FM without ``deterministic`` (the default hot sums are LDS atomics in
arrival order) -- neither repeats from one run to the next, whatever the tree or the build.

usage (GPU box), the other tree being e.g. a ``git worktree`` of the parent commit:
  RFM_LIB_PATH=<this tree>/relevance_factorizationmachine_amd/librfm_hip.so \\
      python tests/manual/fit_bits.py --root <other tree> --out a.npz
  python tests/manual/fit_bits.py --out b.npz
  python tests/manual/fit_bits.py --compare a.npz b.npz
``--root DIR``: the tree whose package and test helpers are imported (default: this one).
``--compare A B`` asserts array_equal key by key."""
import argparse
import os
import sys

import numpy as np

E = 19


def _keep(out, name, model, losses, params):
    for p in params:
        out[f"{name}/{p}"] = getattr(model, p)()
    out[f"{name}/train_loss"], out[f"{name}/val_loss"] = (np.asarray(v, dtype=np.float64) for v in losses)
    out[f"{name}/val_metrics"] = np.asarray(getattr(model, "val_metrics", []), dtype=np.float64)
    print(name, flush=True)


def dump(path):
    import torch.distributed as dist
    from scipy import sparse as sp

    import catalogue_val_common as cv
    import rank_items_common as rk
    import recommend_common as rc
    import relevance_factorizationmachine_amd as pkg
    import test_gpu_catalogue_val as tcv
    import test_gpu_eval as te
    import test_gpu_fit_dp_eval as tdp
    from conftest import load_golden
    from relevance_factorizationmachine_amd import evaluate, features, recommend, runtime, synth
    from relevance_factorizationmachine_amd.dist import HostStagedTransport, fit_data_parallel

    print("package:", os.path.dirname(pkg.__file__), flush=True)
    rt = runtime.Runtime.get()
    out, default_chunk = {}, evaluate.EvalLoop.CHUNK_BYTES

    def three_per_chunk(frame):
        n_rows, n_groups = len(frame["user"]), np.unique(frame["user"]).shape[0]
        evaluate.EvalLoop.CHUNK_BYTES = 3 * (8 * (n_rows + 3 * n_groups) + 8)

    # ---- FM: no evaluator, ValEvaluator on the device, host callback
    sh = synth.SHAPES["coat"]
    train, val = synth.make_log(sh, "FM", "IPS", seed=0)
    _, val_mf = synth.make_log(sh, "MF", "IPS", seed=0)
    frame = synth.interaction_frame(val_mf, val_mf["features"])
    kw = dict(estimator="IPS", n_epochs=E, n_factors=8, n_features=train["features"].shape[1], lr=1e-4,
              batch_size=500, seed=12345)
    three_per_chunk(frame)
    for name, on_device in (("fm_none", None), ("fm_device", True), ("fm_host", False)):
        hook = None if on_device is None else te._ValEvaluatorLike(dict(frame), {"FM": val["features"]})
        m = pkg.FactorizationMachines(evaluator=hook, **kw)
        m.deterministic, m.device_evaluator = True, bool(on_device)
        _keep(out, name, m, m.fit(train, val), ("V", "w", "w0"))
    evaluate.EvalLoop.CHUNK_BYTES = default_chunk

    # ---- FM: CatalogueValEvaluator every 5 iterations (the fixture models of test_gpu_catalogue_val.py)
    rfm = (pkg, features, recommend, rt)
    gold = (load_golden("recommend"), {layout: load_golden(f"recommend_fm_{layout}") for layout in rc.LAYOUTS})
    train_mask, positives, _ = rk.heldout(gold[0])
    held = (train_mask, positives, sp.csr_matrix(train_mask.astype(np.float64)))
    case = ("coat", 16, 2.0)
    cat = tcv._fm_evaluator(rfm, gold, held, case, every=5)
    m = tcv._fm(rfm, gold, case, E, cat)  # (deterministic)
    _keep(out, "fm_catalogue", m, m.fit(*cv.fixture_split(gold[0], case[0])), ("V", "w", "w0"))
    for metric, table in cat.history.items():
        out[f"fm_catalogue/history_{metric}"] = table

    # ---- fit_data_parallel on one rank, the exchange forced, both exchanges, the device evaluator
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(tdp._free_port()), RFM_DP_FORCE_EXCHANGE="1")
    dist.init_process_group("gloo", rank=0, world_size=1)
    try:
        for ex in ("rows", "dense"):
            m, hook, tr, va, fr, _ = tdp._model("coat_two_users", "IPS", True)  # (deterministic)
            tdp._small_chunks(evaluate, fr)
            losses = fit_data_parallel(m, tr, va, exchange=ex, transport=HostStagedTransport(1, 0, rt=m._rt))
            _keep(out, f"dp_{ex}", m, losses, ("V", "w", "w0"))
            out[f"dp_{ex}/y_score"] = np.asarray(hook.interaction_df["y_score"], dtype=np.float64)
    finally:
        evaluate.EvalLoop.CHUNK_BYTES = default_chunk
        dist.destroy_process_group()

    # ---- MF exact, the device evaluator
    sh = synth.SHAPES["kuairec_small"]
    train, val = synth.make_log(sh, "MF", "IPS", seed=0)
    frame = synth.interaction_frame(val, val["features"])
    three_per_chunk(frame)
    hook = te._ValEvaluatorLike(frame, {"MF": val["features"]})
    m = pkg.LogisticMatrixFactorization(evaluator=hook, estimator="IPS", n_epochs=E, n_factors=16, n_users=sh.n_users,
                                        n_items=sh.n_items, lr=0.01, reg=0.5, batch_size=2000, seed=12345)
    _keep(out, "mf_exact", m, m.fit(train, val), ("P", "Q", "b_u", "b_i"))
    evaluate.EvalLoop.CHUNK_BYTES = default_chunk

    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path}")


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    assert sorted(a.files) == sorted(b.files), "the two files hold different keys"
    differ = [key for key in a.files if not np.array_equal(a[key], b[key], equal_nan=True)]
    print(f"{len(a.files)} arrays, {len(a.files) - len(differ)} bit-identical in both files")
    for key in differ:
        print(f"differs: {key} (max |A - B| = {np.max(np.abs(a[key] - b[key])):.3e})")
    assert not differ, f"{len(differ)} arrays differ"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    args = ap.parse_args()
    if args.compare:
        compare(*args.compare)
    else:
        root = os.path.abspath(args.root)
        sys.path[:0] = [root, os.path.join(root, "tests")]
        dump(args.out)
