"""Exact mini-batch sampler throughput: the device sampler (rfm_sample_batches_device) against the
host sampler (rfm_sample_batches) at 16 threads, in iterations (batches) per second, and a check
that both give the same ids.  One JSON line per (N, B).

    python profiles/sampler_bench.py [--rows 1000000] [--batches 2000 65536] [--iters 200]

Under ``rocprofv3 --kernel-trace --stats`` the per-phase kernel times of the device sampler are
the sample_*_kernel rows."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from relevance_factorizationmachine_amd import runtime  # noqa: E402
from relevance_factorizationmachine_amd.runtime import Runtime, sample_batches, sample_batches_device  # noqa: E402


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--batches", type=int, nargs="+", default=[2000, 65536])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--host-threads", type=int, default=16)
    ap.add_argument("--host-iters", type=int, default=64)
    args = ap.parse_args()
    rt = Runtime.get()
    n = args.rows
    for b in args.batches:
        per_epoch = runtime.sampler_workspace_bytes(n, b)
        group = max(1, min(args.iters, runtime.SAMPLER_WORKSPACE_CAP // per_epoch))
        ws = torch.empty((group * per_epoch,), dtype=torch.uint8, device=rt.torch_device)
        out = rt.empty((args.iters, b), torch.int32)
        sample_batches_device(rt, n, b, 10_000, group, out=out[:group], workspace=ws)  # warm-up
        torch.cuda.synchronize()
        reps = []
        for rep in range(3):
            t0 = time.perf_counter()
            sample_batches_device(rt, n, b, rep * args.iters, args.iters, out=out, workspace=ws)
            torch.cuda.synchronize()
            reps.append(time.perf_counter() - t0)
        dev_s = min(reps)
        t0 = time.perf_counter()
        host = sample_batches(n, b, 2 * args.iters, args.host_iters, n_threads=args.host_threads)
        host_s = time.perf_counter() - t0
        same = bool(np.array_equal(out[: args.host_iters].cpu().numpy(), host))
        print(json.dumps({
            "n_rows": n, "batch_size": b, "iters": args.iters, "epochs_per_group": group,
            "workspace_bytes": group * per_epoch,
            "device_batches_per_s": args.iters / dev_s, "device_us_per_batch": 1e6 * dev_s / args.iters,
            "device_reps_s": reps,
            "host_threads": args.host_threads, "host_iters": args.host_iters,
            "host_batches_per_s": args.host_iters / host_s, "host_us_per_batch": 1e6 * host_s / args.host_iters,
            "device_equals_host": same}), flush=True)
        if not same:
            sys.exit(1)


if __name__ == "__main__":
    main()
