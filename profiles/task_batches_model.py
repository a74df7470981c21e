#!/usr/bin/env python3
"""What the task chains of the FM gradient launch (fm_consume_kernel) have to walk, replayed on the
CPU: log -> hot set -> the plan's slot layout -> marks per task for a few random batches -> how
many batches of four entries (one dependent round trip each) every wavefront runs,

  as the tasks are cut   a lane group runs the marks of its own task: a wavefront runs
                         max over its groups of ceil(marks of the task / 4) batches;
  dealt evenly           the T marks of a workgroup go to its GPB groups in parts of
                         per = ceil(T / GPB) (the empty parts last): a wavefront runs
                         max over its groups of ceil(marks of the part / 4).

The kernel's rules are applied: a workgroup with a task beyond its list (WIN marks) keeps its
tasks, and a plan whose tasks expect no more than one batch (task slots x batch / rows <= 4: small
batches) deals nothing -- both rows are then the same.

A workgroup waits at its barrier for its slowest wavefront and the launch for its slowest
workgroup, so the columns to read are the maximum and the mean over workgroups of their slowest
wavefront, beside the mean per wavefront.  No GPU and no library: the layout loop below is the one
of rfm_fm_plan.hip (hot columns by the default rule, task_words from the expected marks, columns in
ascending order, a column that does not fit into the rest of a workgroup's slots starts at the
next workgroup, a column longer than a workgroup's slots takes whole workgroups).  The batches are
uniform draws without replacement, not the fit's own sampler; the statistics do not depend on it.

usage:  python profiles/task_batches_model.py [--workload kuairec_big] [--batch-size 65536]
                                              [--batches 3] [--factors K]"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from relevance_factorizationmachine_amd import synth  # noqa: E402

K_BLOCK, K_WAVE = 256, 64
K_TASK_MARKS, K_TASK_TRIPS = 8, 1                      # rfm_fm_plan.h, rfm_fm_records.h
K_MAX_HOT, K_HOT_LDS, K_HOT_MIN = 160, 56 << 10, 32    # rfm_fm_plan.h
BATCH = 4                                              # entries per round trip of the chain


def shape_for(k):
    """(lanes per row, factors per lane, chunks per lane): rfm_common.h."""
    vec = 2 if k % 2 == 0 else 1
    units = -(-k // vec)
    lpr = 4
    while lpr < units and lpr < 64:
        lpr *= 2
    nc = 1
    while lpr * nc < units:
        nc *= 2
    return lpr, vec, nc


def layout(lens, n_rows, max_batch, k):
    """First slot of every sparse-class column (-1: hot or empty), slots of a task, of a workgroup,
    number of workgroups, the hot columns."""
    lpr, vec, nc = shape_for(k)
    gpb = K_BLOCK // lpr
    hot = np.zeros(0, dtype=np.int64)
    if nc == 1:
        cand = np.flatnonzero(lens * max_batch >= K_HOT_MIN * n_rows)
        cand = cand[np.argsort(-lens[cand], kind="stable")]
        hot = cand[: min(K_MAX_HOT, K_HOT_LDS // ((k + 2) * 8))]
    marks = (2 if nc > 1 else 1) * K_TASK_MARKS
    W = 1
    while W * 2 * 64 * (max_batch / n_rows) <= 1.5 * marks and W * 2 <= K_TASK_TRIPS * lpr:
        W *= 2
    C, BC = 64 * W, gpb * 64 * W
    is_hot = np.zeros(len(lens), dtype=bool)
    is_hot[hot] = True
    start = np.full(len(lens), -1, dtype=np.int64)
    at = 0
    for c, lc in enumerate(lens):
        lc = int(lc)
        if is_hot[c] or lc == 0:
            continue
        if lc <= BC:
            if lc > BC - at % BC:
                at += BC - at % BC
            start[c] = at
            at += lc
        else:
            at = -(-at // BC) * BC
            start[c] = at
            at += -(-lc // BC) * BC
    return start, C, BC, max(1, -(-at // BC)), hot, gpb, lpr, W


def histogram(x, top):
    h = np.bincount(x, minlength=top + 1)
    return " / ".join(str(int(v)) for v in h)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="kuairec_big", choices=sorted(synth.SHAPES))
    ap.add_argument("--batch-size", type=int, default=65536)
    ap.add_argument("--batches", type=int, default=3)
    ap.add_argument("--factors", type=int, default=0, help="0 = the workload's")
    args = ap.parse_args()
    shape = synth.SHAPES[args.workload]
    k = args.factors or shape.n_factors
    train, _ = synth.make_log(shape, "FM", "IPS", seed=0, n_train=shape.n_train, n_val=16)
    Xc = train["features"].tocsc()
    Xc.sort_indices()
    n_rows, n = Xc.shape
    B = min(args.batch_size, n_rows)
    lens = np.diff(Xc.indptr).astype(np.int64)
    start, C, BC, n_wg, hot, gpb, lpr, W = layout(lens, n_rows, B, k)
    sparse = start >= 0
    # slot of every entry of a sparse-class column, in CSC order (= row order inside a column)
    col_of = np.repeat(np.arange(n), lens)
    keep = sparse[col_of]
    slot = (start[col_of] + (np.arange(Xc.nnz) - Xc.indptr[col_of]))[keep]
    rows = Xc.indices[keep]
    win = 64 if lpr >= 16 else 4 * lpr
    gpw = K_WAVE // lpr  # groups of a wavefront
    print(f"{shape.name}: {n_rows} rows x {n} columns, {Xc.nnz / n_rows:.1f} entries per row, k = {k} "
          f"({lpr} lanes per row, {gpb} groups per workgroup, list of {win}), batch {B}")
    print(f"hot columns {len(hot)}, task_words {W} ({C} slots per task, {BC} per workgroup), "
          f"{n_wg} task workgroups, {n_wg * gpb} tasks, {int(sparse.sum())} sparse-class columns "
          f"({int((lens[sparse] > BC).sum())} longer than a workgroup)")
    rng = np.random.default_rng(0)
    for b in range(args.batches):
        in_batch = np.zeros(n_rows, dtype=bool)
        in_batch[rng.permutation(n_rows)[:B]] = True
        marked = slot[in_batch[rows]]
        per_task = np.bincount(marked // C, minlength=n_wg * gpb).reshape(n_wg, gpb)
        T = per_task.sum(axis=1)
        per = -(-T // gpb)
        part = np.clip(T[:, None] - np.arange(gpb)[None, :] * per[:, None], 0, per[:, None])
        over = (per_task > win).any(axis=1)
        print(f"\nbatch {b}: {int(T.sum())} marks; per task mean {per_task.mean():.2f} max {int(per_task.max())}; "
              f"per workgroup mean {T.mean():.1f} max {int(T.max())} (dealt evenly: at most {int(per.max())} per group); "
              f"workgroups with a task over its list: {int(over.sum())}")
        pools = C * B > BATCH * n_rows  # consume_pools (rfm_fm_kernels.hpp)
        if not pools:
            print(f"  (a task expects {C * B / n_rows:.1f} marks, one batch at most: this plan deals nothing)")
        dealt = np.where(over[:, None] | (not pools), per_task, part)
        for name, marks in (("as the tasks are cut", per_task), ("dealt evenly", dealt)):
            waves = (-(-marks // BATCH)).reshape(n_wg, gpb // gpw, gpw).max(axis=2)
            slowest = waves.max(axis=1)
            print(f"  {name:22s} batches of {BATCH} per wavefront: mean {waves.mean():.2f}, max {int(waves.max())}, "
                  f"histogram 0.. {histogram(waves.ravel(), int(waves.max()))}; mean over workgroups of their "
                  f"slowest wavefront {slowest.mean():.2f}")


if __name__ == "__main__":
    main()
