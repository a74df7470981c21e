#!/usr/bin/env python3
"""Per-kernel times of `tests/manual/rank_catalogue_timing.py --device-only PLAN.json` from its
rocprofv3 kernel trace (profiles/rank_catalogue_prof.sh).  Per configuration: rfm_pair_topk at
k = 64 (`pair_tile_kernel<1>` + `topk_merge_kernel`: the floor, one pass over the product plus a
ranking) and per depth the two stages of rfm_pair_order -- `pair_tile_kernel<4>` (the raw logits
to the workspace) and `order_rows_kernel` (one launch per page of 4 096 ranks, summed) -- with
their sum as a multiple of the floor, and the registers of the kernels.
usage: python profiles/rank_catalogue_trace_summary.py <kernel_trace.csv> <PLAN.json>"""
import csv
import json
import sys


def main():
    rows = sorted(csv.DictReader(open(sys.argv[1])), key=lambda r: int(r["Start_Timestamp"]))
    plan = json.load(open(sys.argv[2]))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    is_mode = lambda r, m: "pair_tile_kernel" in r["Kernel_Name"] and any(  # noqa: E731
        s in r["Kernel_Name"] for s in (f"<{m}>", f"ILi{m}E", f"({m})"))
    tile = [r for r in rows if is_mode(r, 1) or is_mode(r, 4)]
    rank = [r for r in rows if "topk_merge_kernel" in r["Kernel_Name"] or "order_rows_kernel" in r["Kernel_Name"]]
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    for name, pick in (("pair_tile_kernel<1>", lambda r: is_mode(r, 1)), ("pair_tile_kernel<4>", lambda r: is_mode(r, 4)),
                       ("order_rows_kernel", lambda r: "order_rows_kernel" in r["Kernel_Name"])):
        first = next((r for r in rows if pick(r)), None)
        if first:
            print(f"{name}: " + ", ".join(f"{key} {first[key]}" for key in
                  ("VGPR_Count", "Accum_VGPR_Count", "SGPR_Count", "LDS_Block_Size", "Scratch_Size") if key in first))
    at_t = at_r = 0
    floor, config = None, None
    for step in plan:
        a, b = [], []
        for _ in range(step["calls"]):
            a.append(sum(us(r) for r in tile[at_t:at_t + step["tile"]]))
            b.append(sum(us(r) for r in rank[at_r:at_r + step["rank"]]))
            at_t += step["tile"]
            at_r += step["rank"]
        a, b = med(a), med(b)
        if step["config"] != config:
            config = step["config"]
            print(config)
        if "topk" in step["what"]:
            floor = a + b
            print(f"    {step['what']}: tile {a:.1f} us + merge {b:.1f} us = {floor:.1f} us")
        else:
            print(f"    {step['what']}: stage 1 (logits) {a:.1f} us + stage 2 (ranking, {step['rank']} page(s)) {b:.1f} us "
                  f"= {a + b:.1f} us = {(a + b) / floor:.2f} x rfm_pair_topk k=64; stage 2 share {100 * b / (a + b):.0f} %")
    assert at_t == len(tile) and at_r == len(rank), (at_t, len(tile), at_r, len(rank))


if __name__ == "__main__":
    main()
