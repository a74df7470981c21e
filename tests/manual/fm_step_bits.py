#!/usr/bin/env python3
"""Every array the FM step's gradient side produces on the case lists of tests/test_gpu_grad_forms.py,
in one .npz, to compare two builds of the library bit for bit:

  <case>/grad_full, grad_shard         rfm_fm_grad of the whole log (shuffled) and of a five-row shard
  <case>/rows_full, rows_shard, gw0_*  the records and g_w0 of rfm_fm_grad_rows of the same
  <case>/V, w, w0                      the parameters after three rfm_fm_step calls (whole log, its
                                       first half, whole log) on the same plan, after the gradients

The cases: every (k, hot) of CASES_A for which every sum of a step has a fixed order (hot_min_count
-1 and -2 at every one-chunk class, the chunked classes at 0), and both forms, short and long, of
every CASES_B case (split columns: the finalize launch).  The default-mode cases (hot 0 or 4 at
one chunk per lane) are left out: their hot sums are LDS atomics in the forward and do not repeat
from one run to the next, whatever the build.

usage (GPU box):
  RFM_LIB_PATH=<other build>/librfm_hip.so python tests/manual/fm_step_bits.py --out a.npz
  python tests/manual/fm_step_bits.py --out b.npz
  python tests/manual/fm_step_bits.py --compare a.npz b.npz
`--compare A B` asserts array_equal key by key."""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import grad_forms_common as gf  # noqa: E402
import test_gpu_grad_forms as tg  # noqa: E402

LR = 2.0 ** -10


def run_case(rt, out, name, log, k, hot, theta, full, shard):
    dev = gf.DeviceLog(rt, log, k, len(full), hot)
    try:
        params = gf.Params(rt, *theta)
        for tag, ids in (("full", full), ("shard", shard)):
            out[f"{name}/grad_{tag}"], _ = gf.dense_grad(dev, ids, params)
            rec = gf.grad_rows(dev, ids, params, dev.n)
            out[f"{name}/rows_{tag}"], out[f"{name}/gw0_{tag}"] = rec.filled(), np.float64(rec.gw0)
        for ids in (full, full[: len(full) // 2], full):
            gf.step(dev, ids, params, LR)
        out[f"{name}/w0"], out[f"{name}/w"], out[f"{name}/V"] = params.host()
        return dev.plan.info()
    finally:
        dev.close()


def dump(path):
    from relevance_factorizationmachine_amd import runtime
    rt = runtime.Runtime.get()
    out = {}
    for k, hot in tg.CASES_A:
        if not gf.fixed_order(k, hot):
            continue
        log = tg._log_a(k >= 500)
        n_rows, n = log["features"].shape
        full = np.random.default_rng(k).permutation(n_rows).astype(np.int32)
        run_case(rt, out, f"A-{gf.class_id(k)}-hot{hot}", log, k, hot, gf.perturbed_init(k, n, k), full,
                 tg.SHARD % n_rows)
        print(gf.class_id(k), hot, flush=True)
    for k, hot in gf.CASES_B:
        for form in ("short", "long"):
            bc = tg._workgroup_slots(k)
            n_rows = (bc if form == "short" else tg.K_SHORT_SPLIT * bc) + 37
            log, theta, full, shard = gf.split_case(k, n_rows, 24 if n_rows > 5000 else 60, 1, 7 * k + len(form))
            info = run_case(rt, out, f"B-{gf.class_id(k)}-hot{hot}-{form}", log, k, hot, theta, full, shard)
            assert info["split_columns"] >= 1
            print(gf.class_id(k), hot, form, flush=True)
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
    args = ap.parse_args()
    if args.compare:
        compare(*args.compare)
    else:
        dump(args.out)
