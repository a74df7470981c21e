#!/usr/bin/env python3
"""Every array the exact MF batch step produces on the case list of tests/mf_step_common.py, in one
.npz, to compare two builds of the library bit for bit:

  <case>/levels_ex/{P,Q,b_u,b_i}   rfm_mf_sgd_levels_ex on every case of step_cases() and the grid_case of
                                   every GRID_KS
  <case>/levels/...                rfm_mf_schedule + rfm_mf_sgd_levels on the same cases (the launches are
                                   those of launch_plan(..., "levels"))
  <case>/hogwild/...               rfm_mf_sgd_hogwild where no row is shared (the grid cases)
  predict-k<k>-n<rows>-ids<0|1>/{pred,fused,loss}   the scoring problems of predict_sizes

usage (GPU box):
  RFM_LIB_PATH=<other build>/librfm_hip.so python tests/manual/mf_step_bits.py --out a.npz
  python tests/manual/mf_step_bits.py --out b.npz
  python tests/manual/mf_step_bits.py --compare a.npz b.npz
`--compare A B` asserts array_equal key by key; where a `levels` or `hogwild` array of B differs from
A's it must equal B's own `levels_ex` array of the same case, which is reported, and anything else
fails."""
import argparse
import dataclasses
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import mf_step_common as ms  # noqa: E402

NAMES = ("P", "Q", "b_u", "b_i")


def dump(path):
    import torch

    from relevance_factorizationmachine_amd import runtime
    rt = runtime.Runtime.get()
    n_cu = int(torch.cuda.get_device_properties(rt.device).multi_processor_count)
    out = {}

    def keep(case, entry, arrays):
        for nm, a in zip(NAMES, arrays):
            out[f"{case.name}/{entry}/{nm}"] = a

    cases = list(ms.step_cases().values()) + [ms.grid_case(k, n_cu) for k in ms.GRID_KS]
    for case in cases:
        sched, init = ms.reach(case), case.init()
        keep(case, "levels_ex", ms.run_levels_ex(rt, case, sched, init))
        if "levels" not in case.want_plan:  # run_levels asserts the plan the case names; these name none
            _, lptr = runtime.mf_schedule(case.users, case.items, case.n_users, case.n_items)
            case = dataclasses.replace(case, want_plan={**case.want_plan, "levels": ms.launch_plan(lptr, case.k, "levels")})
        keep(case, "levels", ms.run_levels(rt, case, init))
        if ms.is_disjoint(case.pairs):
            keep(case, "hogwild", ms.run_hogwild(rt, case, init))
        print(case.name, flush=True)
    for k in (lo for lo, _ in ms.CLASS_RANGE.values()):
        for n_rows in ms.predict_sizes(k, n_cu):
            for with_ids in (False, True):
                prob = ms.predict_problem(k, n_rows, with_ids)
                key = f"predict-k{k}-n{n_rows}-ids{int(with_ids)}"
                out[key + "/pred"], _ = ms.run_predict(rt, prob, loss=False)
                out[key + "/fused"], loss = ms.run_predict(rt, prob, loss=True)
                out[key + "/loss"] = np.float64(loss)
        print(f"predict k{k}", flush=True)
    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path}")


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    assert sorted(a.files) == sorted(b.files), "the two files hold different keys"
    via_ex = []
    for key in a.files:
        if np.array_equal(a[key], b[key], equal_nan=True):
            continue
        case, entry, nm = key.split("/")
        assert entry in ("levels", "hogwild"), f"{key} differs"
        assert np.array_equal(b[key], b[f"{case}/levels_ex/{nm}"]), f"{key} differs from A and from B's levels_ex"
        via_ex.append(key)
    print(f"{len(a.files)} arrays, {len(a.files) - len(via_ex)} bit-identical in both files")
    for key in via_ex:
        print(f"differs from A, equals B's levels_ex: {key} (max |A - B| = {np.max(np.abs(a[key] - b[key])):.3e})")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    args = ap.parse_args()
    if args.compare:
        compare(*args.compare)
    else:
        dump(args.out)
