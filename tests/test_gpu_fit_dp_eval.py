"""The ValEvaluator on the device inside ``dist.fit_data_parallel`` (``rfm_fm_fit_dp_eval``): 1, 2
and 3 ranks each score and rank only the rows of their share of the user groups, the per-user
tables meet in one all-gather per run of iterations, and every rank reports the metric list the
host callback -- and the single-process ``fit()`` -- gives, without calling the evaluator once.

The ranks share the box's one GPU, so the collectives go through the C ABI's ``rfm_transport``
callbacks (host-staged gloo); the RCCL form of the same all-gather (transport=None, one GPU per
rank) needs a multi-GPU node and is NOT covered here."""
import os
import socket

import numpy as np
import pytest

from conftest import rel_err
from relevance_factorizationmachine_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-12
# name: (shape, n_factors, batch, iterations, lr, alpha, frame); frame "unique" = first occurrences
# of every (user, item) pair (no repeated features: no tie with small initial parameters), "all" =
# every row (repeated pairs tie exactly: users redone on the host), "two_users" = the rows of two
# users only (with three ranks one rank holds no group)
CASES = {
    "k16": ("kuairec_small", 16, 2000, 5, 1e-4, 0.05, "unique"),
    # the published point; 10 815 rows take the sliced forward, three ranks' shards of ~3 600 rows
    # alone would not (RFM_SLICED_MIN_ROWS = 4 096): they must score in the whole log's form
    "k400": ("kuairec_small", 400, 2000, 3, 9e-6, 0.05, "unique"),
    "ties": ("kuairec_small", 16, 2000, 5, 9e-6, 2.0, "all"),
    "coat_two_users": ("coat", 8, 500, 7, 1e-4, 2.0, "two_users"),  # 7 iterations, chunks of >= 3
}
CONFIGS = ([(c, est, ex) for c in ("k16", "k400", "ties") for est in ("IPS", "Naive") for ex in ("rows", "dense")]
           + [("coat_two_users", "IPS", "rows"), ("coat_two_users", "Naive", "dense")])


class _ValEvaluatorLike:
    """The attributes of the reference's ValEvaluator (utils/evaluate.py:22-33,160-207); its
    evaluate() counts its calls and restates the metric on the host."""

    metric_name = "DCG"
    rfm_device_evaluator = True  # opts in: its evaluate() IS the reference's metric

    def __init__(self, frame, features, k):
        self.k = k
        self.features = features
        self.interaction_df = dict(frame)
        self._frame = frame
        self.calls = 0

    def evaluate(self, y_scores, estimator):
        from oracle import cpu_ref

        self.calls += 1
        self.interaction_df["y_score"] = np.asarray(y_scores)
        return cpu_ref.val_dcg(self._frame, y_scores, estimator, k=self.k)


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def _setup(case, est):
    shape, k, B, E, lr, alpha, kind = CASES[case]
    sh = synth.SHAPES[shape]
    train, val = synth.make_log(sh, "FM", est, seed=0)
    _, val_mf = synth.make_log(sh, "MF", est, seed=0)
    pairs = val_mf["features"]
    if kind == "unique":
        rows = synth.first_occurrences(pairs)
    elif kind == "two_users":
        top = np.argsort(np.bincount(pairs[:, 0]), kind="stable")[-2:]
        rows = np.flatnonzero(np.isin(pairs[:, 0], top))
    else:
        rows = np.arange(pairs.shape[0])
    frame = synth.interaction_frame({c: v[rows] for c, v in val_mf.items()}, pairs[rows])
    ev_X = val["features"][rows]
    kw = dict(estimator=est, n_epochs=E, n_factors=k, n_features=train["features"].shape[1], lr=lr,
              batch_size=B, seed=12345, alpha=alpha)
    return train, val, frame, ev_X, kw


def _model(case, est, device_evaluator):
    import relevance_factorizationmachine_amd as pkg

    train, val, frame, ev_X, kw = _setup(case, est)
    hook = _ValEvaluatorLike(frame, {"FM": ev_X}, k=16 if case != "coat_two_users" else 5)
    model = pkg.FactorizationMachines(evaluator=hook, **kw)
    model.deterministic = True  # every sum in a fixed order: two fits are bitwise comparable
    model.device_evaluator = device_evaluator
    return model, hook, train, val, frame, ev_X


def _small_chunks(evaluate, frame):
    # chunks of three iterations on one rank (EvalLoop sizing); shards of fewer rows take a few more
    n_rows, n_groups = len(frame["user"]), len(np.unique(frame["user"]))
    evaluate.EvalLoop.CHUNK_BYTES = 3 * (8 * (n_rows + 6 * n_groups) + 16)


def _worker(rank, world, port, out_dir):
    import torch.distributed as dist

    from relevance_factorizationmachine_amd import evaluate
    from relevance_factorizationmachine_amd.dist import HostStagedTransport, fit_data_parallel

    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    old_chunk = evaluate.EvalLoop.CHUNK_BYTES
    try:
        for case, est, ex in CONFIGS:
            res = {}
            for tag, on_device in (("dev", True), ("cb", False)):
                model, hook, train, val, frame, ev_X = _model(case, est, on_device)
                evaluate.EvalLoop.CHUNK_BYTES = old_chunk
                if case == "coat_two_users":
                    _small_chunks(evaluate, frame)
                t = HostStagedTransport(world, rank, rt=model._rt)
                tr, va = fit_data_parallel(model, train, val, exchange=ex, transport=t)
                res.update({f"{tag}_metrics": np.array(model.val_metrics), f"{tag}_calls": hook.calls,
                            f"{tag}_V": model.V(), f"{tag}_w": model.w(), f"{tag}_w0": model.w0(),
                            f"{tag}_tr": np.array(tr), f"{tag}_va": np.array(va),
                            f"{tag}_y_score": np.asarray(hook.interaction_df["y_score"], dtype=np.float64)})
                if on_device:
                    res["host_users"] = model.evaluator_host_users
                    res["host_calls"] = model.evaluator_host_calls
                    got = evaluate.recognise(hook, est)
                    fr = evaluate.DeviceValFrame(model._rt, got[0], got[1], got[2], got[3])
                    res["dcg_of_y"], res["ties_of_y"] = fr.dcg_checked(res["dev_y_score"])
            np.savez(os.path.join(out_dir, f"{case}_{est}_{ex}_rank{rank}.npz"), **res)
    finally:
        evaluate.EvalLoop.CHUNK_BYTES = old_chunk
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [1, 2, 3])
def test_fit_data_parallel_device_evaluator(tmp_path, world):
    import torch.multiprocessing as mp

    from relevance_factorizationmachine_amd import evaluate
    from relevance_factorizationmachine_amd.dist import group_shard_bounds

    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    single = {}
    for case, est, ex in CONFIGS:
        if (case, est) not in single:  # the single-process fit() with the device evaluator
            model, hook, train, val, frame, ev_X = _model(case, est, True)
            old = evaluate.EvalLoop.CHUNK_BYTES
            try:
                if case == "coat_two_users":
                    _small_chunks(evaluate, frame)
                model.fit(train, val)
            finally:
                evaluate.EvalLoop.CHUNK_BYTES = old
            single[(case, est)] = (np.array(model.val_metrics), model.V(),
                                   np.asarray(hook.interaction_df["y_score"], dtype=np.float64), frame)
        want, V1, y1, frame = single[(case, est)]
        E = CASES[case][3]
        outs = [np.load(tmp_path / f"{case}_{est}_{ex}_rank{r}.npz") for r in range(world)]
        what = (case, est, ex, world)
        for o in outs:
            # 1. the evaluator object is never called (the callback path calls it every iteration)
            assert int(o["dev_calls"]) == 0 and int(o["cb_calls"]) == E, what
            assert o["dev_metrics"].shape == (E,), what
            # 2. the callback path's values; training is untouched by the evaluator
            np.testing.assert_allclose(o["dev_metrics"], o["cb_metrics"], rtol=TOL, err_msg=str(what))
            for name in ("V", "w", "w0"):
                np.testing.assert_array_equal(o[f"dev_{name}"], o[f"cb_{name}"], err_msg=str((what, name)))
            for name in ("tr", "va"):  # (a call per iteration vs per run: the loss all-reduce's order differs)
                np.testing.assert_allclose(o[f"dev_{name}"], o[f"cb_{name}"], rtol=TOL, err_msg=str((what, name)))
            # 3. one GPU's values
            np.testing.assert_allclose(o["dev_metrics"], want, rtol=TOL, err_msg=str(what))
            assert rel_err(o["dev_V"], V1) < TOL, what
            # the scores the reference's evaluate() leaves behind: the last iteration's, whole log
            assert rel_err(o["dev_y_score"], y1) < TOL, what
            assert rel_err(o["dev_y_score"], o["cb_y_score"]) < TOL, what
            if case in ("k16", "k400"):
                # tie-free: nothing went to the host, and the metric IS rfm_val_dcg of the whole
                # log's rfm_fm_plan_forward scores, bit for bit (shards scored in the whole log's form)
                assert int(o["host_users"]) == 0 and int(o["ties_of_y"]) == 0, what
                assert float(o["dcg_of_y"]) == float(o["dev_metrics"][-1]), what
            if case == "ties":
                # 4. users whose value hangs on the order of tied scores were redone on the host
                assert int(o["host_users"]) > 0 and int(o["host_calls"]) > 0, what
        for o in outs[1:]:  # every rank holds the same list, bit for bit
            for name in ("dev_metrics", "dev_V", "dev_y_score", "host_users"):
                np.testing.assert_array_equal(outs[0][name], o[name], err_msg=str((what, name)))
        if case == "coat_two_users" and world == 3:
            from relevance_factorizationmachine_amd.evaluate import group_by_user

            _, seg = group_by_user(frame["user"])
            assert np.any(np.diff(group_shard_bounds(seg, world)) == 0)  # 5. a rank without groups
