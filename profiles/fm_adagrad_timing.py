#!/usr/bin/env python3
"""Timing experiment on the GPU box (not part of the product or the tests): microseconds per FM
training step under the SGD rule and under AdaGrad (rfm_fm_plan_set_optimizer).

Two configurations -- the headline (KuaiRec-big shape, k = 32, B = 65 536) and the published point
(k = 400, B = 2 000) --, each rule in fresh processes: one that times K steps wall-clock with nothing
else going on, and one of its own for the kernel times (HIP events around every launch,
rfm_profile_begin / rfm_profile_end; it serialises the launches, so its wall time is not used).
Usage (on the GPU box):
    python profiles/fm_adagrad_timing.py [--root OTHER_TREE] [--rules sgd,adagrad]
``--root``: import the package from another checkout (the parent commit's tree for its SGD step;
such a tree knows no other rule).
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONFIGS = {"headline_k32_B65536": dict(ABL_K="32", ABL_BATCH="65536"),
           "published_k400_B2000": dict(ABL_K="400", ABL_BATCH="2000")}

CHILD = r"""
import ctypes as C, json, os, sys, time
import numpy as np
sys.path.insert(0, %(root)r)
import torch
from relevance_factorizationmachine_amd import _lib, synth
from relevance_factorizationmachine_amd.fm import FactorizationMachines, FmPlan
from relevance_factorizationmachine_amd.runtime import DeviceCSR, Runtime, sample_batches
B = int(os.environ["ABL_BATCH"]); k = int(os.environ["ABL_K"]); K = 40
rule, mode = os.environ["ADA_RULE"], os.environ["ADA_MODE"]
shape = synth.SHAPES["kuairec_big"]
train, _ = synth.make_log(shape, "FM", "IPS", seed=0, n_val=16)
X = train["features"]; n = X.shape[1]
rt = Runtime.get(0)
lr = 9e-6 if rule == "sgd" else 0.05
m = FactorizationMachines(estimator="IPS", n_epochs=1, n_factors=k, lr=lr, batch_size=B, seed=12345, n_features=n)
csr = DeviceCSR(rt, X)
y = rt.upload(train["labels"], dtype=np.float64); p = rt.upload(train["pscores"], dtype=np.float64)
ids = rt.upload(sample_batches(X.shape[0], B, 0, K + 5))
plan = FmPlan(rt, csr, train["labels"], train["pscores"], k, B, 0)
if rule == "adagrad":
    acc = [torch.zeros_like(t.dev) for t in (m.w0, m.w, m.V)]
    plan.set_optimizer(_lib.OPT_ADAGRAD, *acc, 1e-10)
args = (csr.indptr.data_ptr(), csr.indices.data_ptr(), csr.values.data_ptr(), y.data_ptr(), p.data_ptr())
par = (m.w0.dev.data_ptr(), m.w.dev.data_ptr(), m.V.dev.data_ptr())
def run(first, count):
    _lib.check(rt.lib.rfm_fm_train(rt.ctx, plan.handle, *args, ids.data_ptr() + first * B * 4, B, count, *par, lr,
                                   None, None, None, None, None, 0, 1e-8, None, None))
run(0, 5); torch.cuda.synchronize()
out = {"rule": rule, "k": k, "B": B}
if mode == "wall":
    walls = []
    for rep in range(5):
        t0 = time.perf_counter(); run(5, K); torch.cuda.synchronize(); walls.append(1e6 * (time.perf_counter() - t0) / K)
    out["wall_us_per_step"] = sorted(walls)[len(walls) // 2]
    out["wall_us_range"] = [min(walls), max(walls)]
else:
    ms = (C.c_double * 4)(); cnt = (C.c_int64 * 4)()
    _lib.check(rt.lib.rfm_profile_begin(rt.ctx)); run(5, K); _lib.check(rt.lib.rfm_profile_end(rt.ctx, ms, cnt))
    out.update(forward_us=1e3 * ms[0] / max(cnt[0], 1), gradient_us=1e3 * ms[1] / max(cnt[1], 1),
               finalize_us=1e3 * ms[2] / max(cnt[2], 1), step_us=1e3 * ms[3] / max(cnt[3], 1))
assert np.isfinite(m.V.dev.cpu().numpy()).all()
print(json.dumps(out))
"""


def main():
    argv = sys.argv[1:]
    root, rules = ROOT, ["sgd", "adagrad"]
    if "--root" in argv:
        root = os.path.abspath(argv[argv.index("--root") + 1])
    if "--rules" in argv:
        rules = argv[argv.index("--rules") + 1].split(",")
    for name, cfg in CONFIGS.items():
        for rule in rules:
            for mode in ("wall", "kernels"):
                env = dict(os.environ, ADA_RULE=rule, ADA_MODE=mode, **cfg)
                proc = subprocess.run([sys.executable, "-c", CHILD % {"root": root}], env=env, capture_output=True,
                                      text=True, timeout=600)
                if proc.returncode != 0:  # nothing more on the GPU after a failed child
                    print(f"{name} {rule} {mode}: exit {proc.returncode}\n{proc.stderr[-1500:]}", flush=True)
                    sys.exit(1)
                print(f"{name:22s} {proc.stdout.strip().splitlines()[-1]}", flush=True)


if __name__ == "__main__":
    main()
