#!/usr/bin/env python3
"""Per-kernel times of `tests/manual/rank_items_timing.py --device-only` from its rocprofv3 kernel
trace (profiles/rank_items_prof.sh).  Per configuration: the kernel of rfm_pair_scores
(`pair_tile_kernel<0>`, one pass over the product with a store per pair: the floor), and per target
setting the two passes of rfm_pair_ranks -- `pair_tile_kernel<2>` (the targets' logits) and
`pair_tile_kernel<3>` (the counting) -- with their sum as a multiple of the floor, and the
registers of every instantiation of the tile kernel.
usage: python profiles/rank_items_trace_summary.py <kernel_trace.csv> [calls per configuration]"""
import csv
import sys

CONFIGS = [("kuairec_small FM k=32", 1411, 3327, 3), ("kuairec_small FM k=400", 1411, 3327, 3),
           ("kuairec_small MF k=400", 1411, 3327, 3), ("kuairec_big FM k=32", 7176, 10728, 2),
           ("kuairec_big FM k=400", 7176, 10728, 2), ("kuairec_big MF k=400", 7176, 10728, 2)]
SETTINGS = ("10 targets per user", "100 targets per user", "every item")


def main():
    rows = list(csv.DictReader(open(sys.argv[1])))
    calls = int(sys.argv[2]) if len(sys.argv) > 2 else 3
    us = lambda r: (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3  # noqa: E731
    mode = lambda m: [r for r in rows if "pair_tile_kernel" in r["Kernel_Name"]  # noqa: E731
                      and (f"<{m}>" in r["Kernel_Name"] or f"ILi{m}E" in r["Kernel_Name"] or f"({m})" in r["Kernel_Name"])]
    med = lambda v: sorted(v)[len(v) // 2]  # noqa: E731
    scores, logits, counts = mode(0), mode(2), mode(3)
    for m, launches in ((0, scores), (1, mode(1)), (2, logits), (3, counts)):
        if launches:
            r = launches[0]
            print(f"pair_tile_kernel<{m}>: " + ", ".join(f"{key} {r[key]}" for key in
                  ("VGPR_Count", "Accum_VGPR_Count", "SGPR_Count", "LDS_Block_Size", "Scratch_Size") if key in r))
    at_s = at_r = 0
    for name, nu, ni, n_settings in CONFIGS:
        floor = med([us(r) for r in scores[at_s:at_s + calls]])
        at_s += calls
        print(f"{name}: rfm_pair_scores kernel {floor:.1f} us")
        for what in SETTINGS[:n_settings]:
            a = med([us(r) for r in logits[at_r:at_r + calls]])
            b = med([us(r) for r in counts[at_r:at_r + calls]])
            at_r += calls
            print(f"    {what}: logits pass {a:.1f} us, counting pass {b:.1f} us, both {a + b:.1f} us = "
                  f"{(a + b) / floor:.2f} x the rfm_pair_scores kernel")


if __name__ == "__main__":
    main()
