#!/usr/bin/env python3
"""What one catalogue evaluation inside ``fit()`` costs and whether anything synchronises, from the
rocprofv3 traces of ``tests/manual/catalogue_val_timing.py --trace`` (profiles/catalogue_val_prof.sh).

Per kernel of an evaluation -- ``side_sums_kernel`` (FM), the two rank passes ``pair_tile_kernel<2>``
and ``<3>``, ``rank_finish_kernel``, ``rank_metrics_users_kernel``, ``rank_metrics_mean_kernel`` --
the number of launches, the median and the total time, and each one's share of the evaluation's
kernels.  Then, per fit -- ITERS consecutive evaluations (``--trace`` fits evaluate after every one
of their ITERS iterations, so the runs of ``rank_metrics_mean_kernel`` launches cut the trace into
fits) -- the HIP calls that synchronise, copy or set memory and the memory copies that start
between the fit's first and last evaluation.  An FM fit should show ``hipMemsetAsync`` only (the
rank passes clear their outputs); an exact MF fit also shows what it shows without an evaluator:
one asynchronous host-to-device copy of the level schedule per iteration and the producer thread's
event waits.
usage: python profiles/catalogue_val_trace_summary.py <kernel_trace.csv> [<hip_api_trace.csv> [<memory_copy_trace.csv>]] [--iters ITERS]"""
import collections
import csv
import sys

EVAL = ("side_sums_kernel", "pair_tile_kernel<2>", "pair_tile_kernel<3>", "rank_finish_kernel",
        "rank_metrics_users_kernel", "rank_metrics_mean_kernel")
WAITS = ("Synchronize", "hipMemcpy", "hipMemset", "hipStreamWaitEvent", "hipEventQuery", "hipStreamQuery")


def kernel_of(name):
    for m in (2, 3):
        if "pair_tile_kernel" in name and any(s in name for s in (f"<{m}>", f"ILi{m}E", f"({m})")):
            return f"pair_tile_kernel<{m}>"
    return next((k for k in EVAL if "<" not in k and k in name), None)


def main():
    rows = sorted(csv.DictReader(open([a for a in sys.argv[1:] if a.endswith(".csv")][0])), key=lambda r: int(r["Start_Timestamp"]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    by = collections.defaultdict(list)
    for r in rows:
        k = kernel_of(r["Kernel_Name"])
        if k:
            by[k].append(r)
    n_eval = len(by["rank_metrics_mean_kernel"])
    print(f"{n_eval} evaluations in the trace")
    total = sum(us(r) for k in EVAL for r in by[k]) or 1.0
    for k in EVAL:
        v = sorted(us(r) for r in by[k])
        if v:
            regs = ", ".join(f"{key} {by[k][0][key]}" for key in ("VGPR_Count", "Accum_VGPR_Count", "SGPR_Count",
                                                                   "LDS_Block_Size", "Scratch_Size") if key in by[k][0])
            print(f"  {k:28s} {len(v):6d} launches, median {v[len(v) // 2]:9.1f} us, total {sum(v) / 1e3:9.2f} ms, "
                  f"{100 * sum(v) / total:5.1f} % of the evaluations' kernels  [{regs}]")
    print(f"  kernels of one evaluation, mean: {total / max(n_eval, 1):.1f} us")
    args = [a for a in sys.argv[1:] if a.endswith(".csv")]
    iters = int(sys.argv[sys.argv.index("--iters") + 1]) if "--iters" in sys.argv else 20
    if len(args) < 2:
        return
    marks = [int(r["Start_Timestamp"]) for r in by["rank_metrics_mean_kernel"]]
    ends = [int(r["End_Timestamp"]) for r in by["rank_metrics_mean_kernel"]]
    assert len(marks) % iters == 0, (len(marks), iters)
    fits = [(marks[lo], ends[lo + iters - 1], iters) for lo in range(0, len(marks), iters)]
    api = list(csv.DictReader(open(args[1])))
    copies = list(csv.DictReader(open(args[2]))) if len(args) > 2 else []
    for n, (t0, t1, count) in enumerate(fits):
        inside = collections.Counter(r["Function"] for r in api if t0 <= int(r["Start_Timestamp"]) <= t1
                                     and any(w in r["Function"] for w in WAITS))
        moved = collections.Counter(r.get("Direction", "?") for r in copies if t0 <= int(r["Start_Timestamp"]) <= t1)
        print(f"fit {n}: {count} evaluations over {(t1 - t0) / 1e6:.2f} ms; between the first and the last: "
              f"HIP calls that wait, copy or set {dict(inside) or 'none'}; memory copies {dict(moved) or 'none'}")


if __name__ == "__main__":
    main()
