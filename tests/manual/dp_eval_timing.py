#!/usr/bin/env python3
"""Wall time per iteration of `fit_data_parallel` with a ValEvaluator: computed on the device inside
the library's loop (`rfm_fm_fit_dp_eval`) against the host callback per iteration
(`device_evaluator = False`), at the reference's published point (KuaiRec-small shape, k = 400,
B = 2 000, the whole validation frame as the evaluation log, k = 50 ranking positions).
The ranks share ONE GPU and talk through the host-staged transport: the numbers compare the two
evaluator paths under that setup; they are not a scaling measurement.
usage (GPU box): python tests/manual/dp_eval_timing.py [world] [iterations]"""
import os
import socket
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from relevance_factorizationmachine_amd import synth  # noqa: E402

WORLD = int(sys.argv[1]) if len(sys.argv) > 1 else 2
ITS = int(sys.argv[2]) if len(sys.argv) > 2 else 100


class Hook:
    metric_name = "DCG"
    rfm_device_evaluator = True

    def __init__(self, frame, features):
        self.k, self.features, self.interaction_df, self._frame = 50, features, dict(frame), frame

    def evaluate(self, y_scores, estimator):
        from oracle import cpu_ref

        self.interaction_df["y_score"] = np.asarray(y_scores)
        return cpu_ref.val_dcg(self._frame, y_scores, estimator, k=self.k)


def make(on_device, its):
    import relevance_factorizationmachine_amd as pkg

    sh = synth.SHAPES["kuairec_small"]
    train, val = synth.make_log(sh, "FM", "IPS", seed=0)
    _, val_mf = synth.make_log(sh, "MF", "IPS", seed=0)
    frame = synth.interaction_frame(val_mf, val_mf["features"])
    model = pkg.FactorizationMachines(estimator="IPS", n_epochs=its, n_factors=400, lr=9e-6, batch_size=2000,
                                      seed=12345, n_features=train["features"].shape[1],
                                      evaluator=Hook(frame, {"FM": val["features"]}))
    model.device_evaluator = on_device
    return model, train, val


def worker(rank, world, port):
    import torch.distributed as dist

    from relevance_factorizationmachine_amd.dist import HostStagedTransport, fit_data_parallel

    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        for on_device in (True, False):
            for its in (2, ITS):  # (the first fit warms up: library load, kernels, plan cache)
                model, train, val = make(on_device, its)
                t = HostStagedTransport(world, rank, rt=model._rt)
                dist.barrier()
                t0 = time.perf_counter()
                fit_data_parallel(model, train, val, exchange="auto", transport=t)
                model._rt.sync()
                dt = time.perf_counter() - t0
            if rank == 0:
                path = "device evaluator (rfm_fm_fit_dp_eval)" if on_device else "host callback per iteration"
                extra = (f", {model.evaluator_host_calls} iterations with host-resolved users"
                         if on_device else "")
                print(f"world {world}, ranks sharing one GPU, {path}: {1e3 * dt / ITS:.3f} ms per iteration "
                      f"over {ITS} iterations (last metric {model.val_metrics[-1]:.6f}{extra})", flush=True)
    finally:
        dist.destroy_process_group()


if __name__ == "__main__":
    import torch.multiprocessing as mp

    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    mp.spawn(worker, args=(WORLD, port), nprocs=WORLD, join=True)
