"""Timing of MF fold-in on one GPU: what profiles/n13/fold_in_timing.txt records.

  a. the reference's KuaiRec catalogue shape: 10 728 items, 7 176 new users whose chain lengths are
     log-normal (median 60, clipped at 5 000: about a million examples), k = 400 and k = 32, 1 and 5
     passes;
  b. a single new user with a chain of 1 000 examples.

Per case: the kernel alone (HIP events around rfm_mf_fold_in on uploaded arrays, median of the
repeats), one whole ``fold_in_users`` call (host grouping, uploads, launch, synchronise), and the
NumPy float64 loop on the CPU (b. in full; a. on the longest chains and a sample, scaled by examples).
For b. the time per example is the dependent chain's step; for a. the kernel time stands beside the
longest chain times that step, the bound no schedule of independent chains can beat.

    python profiles/fold_in_timing.py --out profiles/n13/fold_in_timing.txt

The file is this script's output and nothing else: a run overwrites it.  It ends with the chain's
step beside the yardstick of the MF step's sequential kernel and with a.'s distance
from its longest-chain bound.  RFM_LIB_PATH selects another build of the library (a different
RFM_MF_FOLD_READ_AHEAD); the depth in use is read back from rfm_mf_fold_geometry, and what the builds
of other depths gave is kept apart in profiles/n13/read_ahead_depths.txt."""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_ITEMS, N_NEW, LONG = 10728, 7176, 1000
B0, LR, REG = 0.4, 0.02, 0.5


def numpy_row(ids, ry, Q, bi, k, n_passes):
    x, c = np.zeros(k), 0.0
    for _ in range(n_passes):
        for j, r in zip(ids, ry):
            z = x @ Q[j] + c + bi[j] + B0
            err = r - 1.0 / (1.0 + np.exp(-min(max(z, -700.0), 700.0)))
            x = x - LR * (-err * Q[j] + REG * x)
            c = c - LR * (-err + REG * c)
    return x, c


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()

    import torch

    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import _lib
    from relevance_factorizationmachine_amd.fold import fold_examples

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(13)
    lengths = np.clip(rng.lognormal(np.log(60.0), 1.3, size=N_NEW).astype(np.int64), 1, 5000)
    in_tree = os.path.realpath(_lib.LIB_PATH) == os.path.realpath(os.path.join(_lib.PKG_DIR, "librfm_hip.so"))
    say(f"device {torch.cuda.get_device_name(0)}; library {'in-tree' if in_tree else 'another build (RFM_LIB_PATH)'}")
    say(f"a: {N_NEW} new users, {N_ITEMS} items, {int(lengths.sum())} examples, chain lengths median "
        f"{int(np.median(lengths))}, mean {lengths.mean():.0f}, longest {int(lengths.max())}; b: one user, {LONG} examples")

    def log_of(lens):
        n = int(lens.sum())
        users = np.repeat(np.arange(len(lens)), lens)
        return {"features": np.stack([users, rng.integers(0, N_ITEMS, size=n)], axis=1)[rng.permutation(n)],
                "labels": (rng.random(n) < 0.5).astype(np.float64), "pscores": rng.uniform(0.1, 1.0, size=n) ** 0.5}

    logs = {"a": log_of(lengths), "b": log_of(np.array([LONG]))}
    chain, balance, whole, cpu = {}, {}, [], []  # per k: us per example of b., a. over its bound; ms of a call on a.; CPU us
    for k in (400, 32):
        model = pkg.LogisticMatrixFactorization(estimator="IPS", n_epochs=1, n_factors=k, lr=LR, batch_size=1000,
                                                seed=1, n_users=8, n_items=N_ITEMS, reg=REG)
        model.b = B0
        rt = model._rt
        geo = np.zeros(6, dtype=np.int32)
        _lib.check(rt.lib.rfm_mf_fold_geometry(rt.ctx, N_NEW, k, geo.ctypes.data))
        say(f"\nk = {k}: lanes per row {geo[0]}, rows per workgroup {geo[3]}, workgroups {geo[4]}, read-ahead depth {geo[5]}")
        Q, bi = model.Q(), model.b_i()
        step_us = {}
        for name in ("b", "a"):
            data = logs[name]
            n_new = 1 if name == "b" else N_NEW
            row_ptr, ids, ry, order = fold_examples(data, n_new, N_ITEMS, 0, 1)
            dev = [rt.upload(a) for a in (row_ptr, ids, ry, order)]
            longest = int(np.diff(row_ptr).max())
            for n_passes in (1, 5):
                rows = torch.zeros((n_new, k), dtype=torch.float64, device=rt.torch_device)
                bias = torch.zeros((n_new,), dtype=torch.float64, device=rt.torch_device)

                def kernel():
                    rows.zero_()
                    bias.zero_()
                    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    t0.record()
                    _lib.check(rt.lib.rfm_mf_fold_in(rt.ctx, *(d.data_ptr() for d in dev), n_new, model.Q.dev.data_ptr(),
                                                     model.b_i.dev.data_ptr(), N_ITEMS, B0, k, LR, REG, n_passes,
                                                     rows.data_ptr(), bias.data_ptr()))
                    t1.record()
                    t1.synchronize()
                    return t0.elapsed_time(t1) * 1e3

                def call():
                    rt.sync()
                    t = time.perf_counter()
                    folded = model.fold_in_users(data, n_new, n_passes)
                    rt.sync()
                    return (time.perf_counter() - t) * 1e6, folded

                kernel(), call()
                k_us = sorted(kernel() for _ in range(args.repeats))
                c_us = sorted(call()[0] for _ in range(3))
                steps = longest * n_passes
                line = (f"  {name} passes {n_passes}: kernel {k_us[len(k_us) // 2]:10.1f} us (min {k_us[0]:.1f}, max {k_us[-1]:.1f}); "
                        f"whole call {c_us[1]:10.1f} us")
                if name == "b":
                    step_us[n_passes] = k_us[len(k_us) // 2] / steps
                    chain.setdefault(k, []).append(step_us[n_passes])
                    line += f"; {step_us[n_passes]:.3f} us per example of the chain"
                else:
                    bound = steps * step_us[n_passes]
                    balance.setdefault(k, []).append(k_us[len(k_us) // 2] / bound)
                    whole.append(c_us[1] / 1e3)
                    line += (f"; longest chain {longest} x {n_passes} x {step_us[n_passes]:.3f} us = {bound:.1f} us: "
                             f"{k_us[len(k_us) // 2] / bound:.2f} times the bound")
                say(line)
                if args.no_cpu or n_passes == 5 and name == "a":
                    continue
                got_rows, got_bias = call()[1].numpy()
                t = time.perf_counter()
                if name == "b":
                    x, c = numpy_row(ids, ry, Q, bi, k, n_passes)
                    cpu_us = (time.perf_counter() - t) * 1e6
                    cpu.append(cpu_us / steps)
                    worst = np.abs(got_rows[0] - x).max() / np.abs(x).max()
                    say(f"      NumPy float64 loop: {cpu_us:.0f} us ({cpu_us / steps:.2f} us per example); device rows within "
                        f"{worst:.1e} of it")
                else:
                    sample = np.concatenate([order[:3], order[:: max(1, n_new // 60)]])
                    done, worst = 0, 0.0
                    for r in sample:
                        sl = slice(row_ptr[r], row_ptr[r + 1])
                        x, _ = numpy_row(ids[sl], ry[sl], Q, bi, k, n_passes)
                        done += sl.stop - sl.start
                        worst = max(worst, np.abs(got_rows[r] - x).max() / np.abs(x).max())
                    cpu_us = (time.perf_counter() - t) * 1e6
                    cpu.append(cpu_us / done)
                    say(f"      NumPy float64 loop on {len(sample)} users ({done} examples): {cpu_us / done:.2f} us per example, "
                        f"{cpu_us / done * row_ptr[-1] / 1e6:.2f} s for all of them on one core (scaled); device rows within "
                        f"{worst:.1e} of it")

    def span(v, fmt="{:.2f}"):
        return fmt.format(min(v)) if min(v) == max(v) else f"{fmt.format(min(v))} - {fmt.format(max(v))}"

    say("\nYardstick: the MF step's sequential kernel runs 0.67 - 1.05 us per level (DESIGN.md 10.4, about 0.25 us of it "
        "the dependent arithmetic); the fold-in chain runs "
        + ", ".join(f"{span(v, '{:.3f}')} us per example at k = {k}" for k, v in chain.items()) + ".")
    say("Balance: a. takes " + ", ".join(f"{span(v)} (k = {k})" for k, v in balance.items())
        + " times its longest chain at that rate.")
    if cpu:
        say(f"CPU: the NumPy float64 loop takes {span(cpu)} us per example on one core.")
    say(f"A whole fold_in_users call on a. is {span(whole, '{:.0f}')} ms (host grouping of a million examples, uploads, "
        f"launch, synchronise).")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
