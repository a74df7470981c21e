#!/usr/bin/env python3
"""Per-kernel times of `tests/manual/recommend_timing.py --only-b` from its rocprofv3 kernel trace
(profiles/recommend_prof.sh): the pair tile, the merge and the two side-sum launches of every
recommend() call, and the tile kernel's achieved f64 GFLOP/s = 2 n_users n_items kpad / its time.
usage: python profiles/recommend_trace_summary.py <kernel_trace.csv> [calls per configuration]"""
import csv
import sys

CONFIGS = [("kuairec_small FM k=32", 1411, 3327, 32, True), ("kuairec_small FM k=400", 1411, 3327, 400, True),
           ("kuairec_small MF k=400", 1411, 3327, 400, False), ("kuairec_big FM k=32", 7176, 10728, 32, True),
           ("kuairec_big FM k=400", 7176, 10728, 400, True), ("kuairec_big MF k=400", 7176, 10728, 400, False)]


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    pick = lambda name: [r for r in rows if name in r["Kernel_Name"]]  # noqa: E731
    tile, merge, side = pick("pair_tile_kernel"), pick("topk_merge_kernel"), pick("side_sums_kernel")
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else len(tile) // len(CONFIGS)
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    at_tile = at_side = 0
    for name, nu, ni, k, is_fm in CONFIGS:
        t = [us(r) for r in tile[at_tile:at_tile + calls]]
        m = [us(r) for r in merge[at_tile:at_tile + calls]]
        s = [us(a) + us(b) for a, b in zip(side[at_side:at_side + 2 * calls:2], side[at_side + 1:at_side + 2 * calls:2])] if is_fm else [0.0]
        r0 = tile[at_tile]
        at_tile += calls
        at_side += 2 * calls if is_fm else 0
        kpad = (k + 3) // 4 * 4
        total = med(t) + med(m) + med(s)
        print(f"{name}: side sums {med(s):.1f} us ({100 * med(s) / total:.0f} %), pair tile {med(t):.1f} us "
              f"({100 * med(t) / total:.0f} %), merge {med(m):.1f} us ({100 * med(m) / total:.0f} %); tile kernel "
              f"{2 * nu * ni * kpad / (med(t) * 1e-6) / 1e9:.0f} GFLOP/s f64; {int(r0['Grid_Size_X']) // int(r0['Workgroup_Size_X'])} x "
              f"{r0['Grid_Size_Y']} workgroups, {calls} calls")


if __name__ == "__main__":
    main()
