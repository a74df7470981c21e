#!/usr/bin/env python3
"""Timing experiment on the GPU box (not part of the product or the tests): the exact MF batch step
under the SGD rule and under AdaGrad (rfm_mf_sgd_levels_opt), at k = 16, 128, 400.

Per level: one chain of 1 000 levels through one cached item with a new user at every level (the
user rows are read ahead, the item row and its accumulators live in LDS): one sequential launch,
wall-clock over 30 calls with nothing else going on, divided by the levels.  Per fit() iteration:
``LogisticMatrixFactorization.fit`` on the kuairec_small log (B = 2 000, 40 iterations), wall-clock
of the whole call divided by the iterations (schedule thread, copies, the two loss launches and the
step together).  Each (k, rule) in a fresh process.
Usage (on the GPU box):
    python profiles/mf_adagrad_timing.py [--root OTHER_TREE] [--rules sgd,adagrad]
``--root``: import the package from another checkout (the parent commit's tree for its SGD step;
such a tree knows no other rule).
"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (16, 128, 400)

CHILD = r"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, %(root)r)
import torch
from relevance_factorizationmachine_amd import _lib, synth
from relevance_factorizationmachine_amd.mf import LogisticMatrixFactorization
from relevance_factorizationmachine_amd.runtime import Runtime, mf_cache_capacity, mf_schedule_ex
k = int(os.environ["ADA_K"]); rule = os.environ["ADA_RULE"]
rt = Runtime.get(0)
L = 1000
users = np.arange(1, L + 1, dtype=np.int64); items = np.ones(L, dtype=np.int64)
rng = np.random.default_rng(0)
y = (rng.random(L) < 0.5).astype(np.float64); p = rng.uniform(0.1, 1.0, L) ** 0.5
ex, lptr, cache = mf_schedule_ex(users, items, y, p, L + 2, 3, mf_cache_capacity(k))
assert len(lptr) - 1 == L and len(cache) == 1
lim = 4 * np.sqrt(6 / k)
dev = [rt.upload(a) for a in (rng.uniform(-lim, lim, (L + 2, k)), rng.uniform(-lim, lim, (3, k)),
                              rng.normal(0, 1e-3, L + 2), rng.normal(0, 1e-3, 3))]
acc = [torch.zeros_like(t) for t in dev]
d_ex = rt.upload(np.ascontiguousarray(ex).view(np.uint8)); d_lptr = rt.upload(lptr); d_cache = rt.upload(cache)
head = (rt.ctx, d_ex.data_ptr(), lptr.ctypes.data, d_lptr.data_ptr(), L, d_cache.data_ptr(), 1,
        *(t.data_ptr() for t in dev), 0.4, k, 0.02, 0.5)
def step():
    if rule == "sgd":
        _lib.check(rt.lib.rfm_mf_sgd_levels_ex(*head))
    else:
        _lib.check(rt.lib.rfm_mf_sgd_levels_opt(*head, 1, *(t.data_ptr() for t in acc), 1e-10))
for _ in range(5):
    step()
torch.cuda.synchronize()
walls = []
for rep in range(5):
    t0 = time.perf_counter()
    for _ in range(30):
        step()
    torch.cuda.synchronize()
    walls.append(1e6 * (time.perf_counter() - t0) / 30 / L)
out = {"rule": rule, "k": k, "us_per_level": sorted(walls)[2], "us_per_level_range": [min(walls), max(walls)]}
assert all(np.isfinite(t.cpu().numpy()).all() for t in dev)
sh = synth.SHAPES["kuairec_small"]
train, val = synth.make_log(sh, "MF", "IPS", seed=0)
fits = []
for rep in range(3):
    m = LogisticMatrixFactorization(estimator="IPS", n_epochs=40, n_factors=k, n_users=sh.n_users, n_items=sh.n_items,
                                    lr=0.01 if rule == "sgd" else 0.05, reg=0.5, batch_size=2000, seed=12345)
    if rule != "sgd":
        m.optimizer = rule
    t0 = time.perf_counter(); m.fit(train, val); fits.append(1e6 * (time.perf_counter() - t0) / 40)
out.update(us_per_fit_iteration=sorted(fits)[1], us_per_fit_iteration_range=[min(fits), max(fits)])
print(json.dumps(out))
"""


def main():
    argv = sys.argv[1:]
    root, rules = ROOT, ["sgd", "adagrad"]
    if "--root" in argv:
        root = os.path.abspath(argv[argv.index("--root") + 1])
    if "--rules" in argv:
        rules = argv[argv.index("--rules") + 1].split(",")
    for k in KS:
        for rule in rules:
            env = dict(os.environ, ADA_RULE=rule, ADA_K=str(k))
            proc = subprocess.run([sys.executable, "-c", CHILD % {"root": root}], env=env, capture_output=True,
                                  text=True, timeout=600)
            if proc.returncode != 0:  # nothing more on the GPU after a failed child
                print(f"k={k} {rule}: exit {proc.returncode}\n{proc.stderr[-1500:]}", flush=True)
                sys.exit(1)
            print(proc.stdout.strip().splitlines()[-1], flush=True)


if __name__ == "__main__":
    main()
