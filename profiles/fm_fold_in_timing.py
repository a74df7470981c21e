"""Timing of FM fold-in on one GPU: what profiles/n16/fm_fold_in_timing.txt records.

The case is N13's a.: the reference's KuaiRec catalogue shape, 10 728 items, 7 176 new users whose
example counts are log-normal (median 61, clipped at 5 000: about a million examples), at k = 32 and
k = 400, for 1 and 5 passes.  The catalogue is coat-shaped ([one-hot user | user table | one-hot item
| item table]); the new users bring their table rows and no id column.

Per case: the kernel alone (HIP events around rfm_fm_fold_in on arrays that are already on the device,
median of the repeats), one whole ``fold_in_users`` call (host grouping, uploads, the fixed side's and
the new rows' side sums, launch, synchronise) with and without ``ops=``, the longest row alone (one
workgroup: what the launch cannot go below while a row is one workgroup's), and two yardsticks:

  * the NumPy float64 restatement of the rule on one CPU core (a sample of rows, scaled by examples);
  * the gather bound: every example reads one row of the fixed side, examples x k x 8 bytes per pass,
    at the L2 gather rate DESIGN.md 4 / 6 records (16.8 - 18.8 TB/s; the lower figure is used).

    python profiles/fm_fold_in_timing.py --out profiles/n16/fm_fold_in_timing.txt

The file is this script's output and nothing else: a run overwrites it."""
import argparse
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_ITEMS, N_NEW, N_OLD, UW, IW = 10728, 7176, 8, 16, 16
LR = 1e-5
L2_GATHER = 16.8e12  # bytes per second, DESIGN.md 6


def numpy_row(ids, ry, F, fL, g, l, c, k, n_passes):
    """The rule of one row in float64, vectorised over the row's examples (no BLAS: one core)."""
    Fj, fl = F[ids, :k], fL[ids]
    h = g + Fj
    nu, om = np.zeros(k), 0.0
    gF = (g * Fj).sum(axis=1)
    for _ in range(n_passes):
        z = c + l + fl + gF + om + (nu * h).sum(axis=1)
        err = ry - 1.0 / (1.0 + np.exp(-np.clip(z, -700.0, 700.0)))
        om = om + LR * err.sum()
        nu = nu + LR * (err[:, None] * h).sum(axis=0)
    return nu, om


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--no-cpu", action="store_true")
    args = ap.parse_args()

    import torch

    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import _lib
    from relevance_factorizationmachine_amd import recommend as rec
    from relevance_factorizationmachine_amd.fold import fold_examples
    from relevance_factorizationmachine_amd.runtime import DeviceCSR

    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    rng = np.random.default_rng(13)
    lengths = np.clip(rng.lognormal(np.log(60.0), 1.3, size=N_NEW).astype(np.int64), 1, 5000)
    n_ex = int(lengths.sum())
    say(f"device {torch.cuda.get_device_name(0)}")
    say(f"{N_NEW} new users, {N_ITEMS} items, {n_ex} examples, example counts median {int(np.median(lengths))}, mean "
        f"{lengths.mean():.0f}, longest {int(lengths.max())}")
    users = np.repeat(np.arange(N_NEW), lengths)
    data = {"features": np.stack([users, rng.integers(0, N_ITEMS, size=n_ex)], axis=1)[rng.permutation(n_ex)],
            "labels": (rng.random(n_ex) < 0.5).astype(np.float64), "pscores": rng.uniform(0.1, 1.0, size=n_ex) ** 0.5}

    def table(n, width):
        T = (rng.random((n, width)) < 0.3).astype(np.float64)
        T[:, 0] = 1.0
        return sp.csr_matrix(T)

    n_features = N_OLD + UW + N_ITEMS + IW
    XU = sp.hstack([sp.identity(N_OLD), table(N_OLD, UW), sp.csr_matrix((N_OLD, N_ITEMS + IW))]).tocsr()
    XI = sp.hstack([sp.csr_matrix((N_ITEMS, N_OLD + UW)), sp.identity(N_ITEMS), table(N_ITEMS, IW)]).tocsr()
    new_rows = sp.hstack([sp.csr_matrix((N_NEW, N_OLD)), table(N_NEW, UW), sp.csr_matrix((N_NEW, N_ITEMS + IW))]).tocsr()
    sides = rec.Sides(XU, XI)
    ratios, alone, whole, whole_ops, cpu = {}, {}, [], [], []
    for k in (32, 400):
        model = pkg.FactorizationMachines(estimator="IPS", n_epochs=1, n_factors=k, lr=LR, batch_size=1000, seed=1,
                                          n_features=n_features, alpha=0.3)
        rt = model._rt
        geo = np.zeros(5, dtype=np.int32)
        _lib.check(rt.lib.rfm_fm_fold_geometry(rt.ctx, N_NEW, k, geo.ctypes.data))
        say(f"\nk = {k}: lanes per example {geo[0]}, lane groups per workgroup {geo[3]}, workgroups {geo[4]}")
        ops = rec.operands(model, sides)
        g, l = rec.side_sums(rt, DeviceCSR(rt, new_rows), model.w.dev, model.V.dev, n_features, k)
        row_ptr, ids, ry, order = fold_examples(data, N_NEW, N_ITEMS, 0, 1)
        dev = [rt.upload(a) for a in (row_ptr, ids, ry, order)]
        kp = rec.pad4(k)
        r = int(order[0])
        longest = int(row_ptr[r + 1] - row_ptr[r])
        sl = slice(row_ptr[r], row_ptr[r + 1])
        one = [rt.upload(a) for a in (np.array([0, longest], dtype=np.int64), ids[sl], ry[sl], np.zeros(1, dtype=np.int32))]
        g_one, l_one = g[r: r + 1].contiguous(), l[r: r + 1].contiguous()
        for n_passes in (1, 5):
            V_new = torch.zeros((N_NEW, k), dtype=torch.float64, device=rt.torch_device)
            w_new = torch.zeros((N_NEW,), dtype=torch.float64, device=rt.torch_device)
            A_new, L_new = rt.empty((N_NEW, kp), torch.float64), rt.empty((N_NEW,), torch.float64)

            def kernel(dev=dev, n_new=N_NEW, g=g, l=l):
                V_new.zero_()
                w_new.zero_()
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record()
                _lib.check(rt.lib.rfm_fm_fold_in(
                    rt.ctx, *(d.data_ptr() for d in dev), n_new, g.data_ptr(), l.data_ptr(), ops.B.data_ptr(),
                    ops.LI.data_ptr(), N_ITEMS, model.w0.dev.data_ptr(), k, LR, n_passes, w_new.data_ptr(),
                    V_new.data_ptr(), A_new.data_ptr(), L_new.data_ptr()))
                t1.record()
                t1.synchronize()
                return t0.elapsed_time(t1) * 1e3

            def call(reuse):
                rt.sync()
                t = time.perf_counter()
                folded = model.fold_in_users(sides, new_rows, data, n_passes, ops=ops if reuse else None)
                rt.sync()
                return (time.perf_counter() - t) * 1e6, folded

            kernel(), call(False)
            k_us = sorted(kernel() for _ in range(args.repeats))
            c_us = sorted(call(False)[0] for _ in range(3))
            o_us = sorted(call(True)[0] for _ in range(3))
            med = k_us[len(k_us) // 2]
            bound = n_ex * k * 8 * n_passes / L2_GATHER * 1e6
            ratios.setdefault(k, []).append(med / bound)
            whole.append(c_us[1] / 1e3)
            whole_ops.append(o_us[1] / 1e3)
            say(f"  passes {n_passes}: kernel {med:10.1f} us (min {k_us[0]:.1f}, max {k_us[-1]:.1f}), "
                f"{med * 1e3 / (n_ex * n_passes):.2f} ns per example and pass; gather bound {n_ex * k * 8 * n_passes / 1e6:.0f} MB "
                f"at 16.8 TB/s = {bound:.1f} us: {med / bound:.2f} times the bound; whole call {c_us[1]:10.1f} us, with ops= "
                f"{o_us[1]:10.1f} us")
            # the longest row alone: one workgroup, its lane groups' trips one after the other
            kernel(one, 1, g_one, l_one)
            b_us = sorted(kernel(one, 1, g_one, l_one) for _ in range(args.repeats))[args.repeats // 2]
            trips = -(-longest // int(geo[3]))
            alone.setdefault(k, []).append(b_us / med)
            say(f"      the longest row alone ({longest} examples, {trips} trips of {geo[3]} lane groups a pass): {b_us:.1f} us, "
                f"{b_us / (trips * n_passes):.2f} us per trip: {b_us / med:.2f} of the whole launch")
            if args.no_cpu:
                continue
            got_V, got_w = call(True)[1].numpy()
            F, fL, hg, hl = ops.B.cpu().numpy(), ops.LI.cpu().numpy(), g.cpu().numpy(), l.cpu().numpy()
            c = float(model.w0()[0])
            sample = np.concatenate([order[:3], order[:: max(1, N_NEW // 60)]])
            t = time.perf_counter()
            done, worst = 0, 0.0
            for r in sample:
                sl = slice(row_ptr[r], row_ptr[r + 1])
                nu, _ = numpy_row(ids[sl], ry[sl], F, fL, hg[r, :k], hl[r], c, k, n_passes)
                done += sl.stop - sl.start
                worst = max(worst, np.abs(got_V[r] - nu).max() / np.abs(nu).max())
            cpu_us = (time.perf_counter() - t) * 1e6
            cpu.append(cpu_us * 1e3 / (done * n_passes))
            say(f"      NumPy float64 on {len(sample)} users ({done} examples): {cpu_us * 1e3 / (done * n_passes):.0f} ns per example "
                f"and pass, {cpu_us / done * n_ex / 1e6:.2f} s for all of them on one core (scaled): {cpu_us / done * n_ex / med:.0f} "
                f"times the kernel; device columns within {worst:.1e} of it")

    def span(v, fmt="{:.2f}"):
        return fmt.format(min(v)) if min(v) == max(v) else f"{fmt.format(min(v))} - {fmt.format(max(v))}"

    say("\nGather bound: the kernel takes " + ", ".join(f"{span(v)} (k = {k})" for k, v in ratios.items())
        + " times examples x k x 8 bytes per pass at 16.8 TB/s.")
    say("Longest row: alone it takes " + ", ".join(f"{span(v)} (k = {k})" for k, v in alone.items())
        + " of the whole launch's time.")
    if cpu:
        say(f"CPU: the NumPy float64 restatement takes {span(cpu, '{:.0f}')} ns per example and pass on one core.")
    say(f"A whole fold_in_users call is {span(whole, '{:.0f}')} ms, {span(whole_ops, '{:.0f}')} ms with ops= (host grouping of a "
        f"million examples, the new rows' CSR and side sums, uploads, launch, synchronise).")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
