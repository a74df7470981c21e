"""The AdaGrad rule of the exact MF batch step -- rfm_mf_sgd_levels_opt through the raw C ABI, and
``LogisticMatrixFactorization.optimizer = "adagrad"`` through fit() -- against the long-double
oracle of mf_adagrad_common.py on every case of ``mf_step_common.step_cases()`` (every shape class,
the read-ahead ring on both sides of its boundary, the launch limits, every cache state, seq -> wide
-> seq) and the grid case at the device's CU count, from two accumulator states (G0 = 0, and G0
uniform in [0.25, 4]).  Needs an MI355X: ``pytest -m gpu``.

Every case first asserts, from the library's own host scheduler, the launches and record states it
is named for (``mf_step_common.reach``) and, from ``rfm_mf_opt_geometry``, the class it means.  Every
call is made twice from the same start and must give the same bits.  All eight arrays are held to
the oracle element by element at ``PARAM_TOL`` / ``ACC_TOL`` (derived from a CPU measurement, see
that module); rows of users and items outside the batch, and the sentinels around every array, keep
their bits.  Largest distances an MI355X showed over the case list: see ``GPU_MAX_SEEN`` there."""
import numpy as np
import pytest

import mf_adagrad_common as ma
import mf_step_common as ms
from conftest import assert_elementwise, load_golden, rel_err
from oracle import cpu_ref
from relevance_factorizationmachine_amd import synth

pytestmark = pytest.mark.gpu

TIGHT = 1e-9  # the norm-wise bound of the parity contract (test_gpu_parity.py)
GOLDEN = {"IPS": "mf_adagrad_small", "Naive": "mf_adagrad_small_naive"}


@pytest.fixture(scope="module")
def rt():
    from relevance_factorizationmachine_amd import runtime
    return runtime.Runtime.get()


def _n_cu(rt):
    import torch
    return int(torch.cuda.get_device_properties(rt.device).multi_processor_count)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _same_bits(got, want, what):
    for name, a, b in zip(ma.NAMES, got, want):
        assert np.array_equal(_bits(a), _bits(b)), f"{what}: {name} differs"


def _check(rt, case, kind, want=None):
    sched = ms.reach(case)  # asserts the launches and record states the case is named for
    ma.assert_class(case)
    start = case.init() + ma.acc_init(case, kind)
    want = ma.oracle(case, kind) if want is None else want
    got = ma.run_levels_opt(rt, case, sched, start[:4], start[4:])
    _same_bits(ma.run_levels_opt(rt, case, sched, start[:4], start[4:]), got, f"{case.name} {kind}: two calls")
    worst = ma.assert_all_within(got, want, start, case.pairs, f"{case.name} {kind}")
    print(f"distance {case.name} {kind} parameters {worst[0]:.3e} accumulators {worst[1]:.3e}")
    return got


# --------------------------------------------------------------------------
# 1. every case of the exact step, both accumulator states
# --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ma.ACC_KINDS)
@pytest.mark.parametrize("name", list(ms.step_cases()))
def test_every_case_against_the_oracle(rt, name, kind):
    _check(rt, ms.step_cases()[name], kind)


@pytest.mark.parametrize("kind", ma.ACC_KINDS)
@pytest.mark.parametrize("k", ms.GRID_KS)
def test_wide_level_past_one_pass_of_the_grid(rt, k, kind):
    _check(rt, ms.grid_case(k, _n_cu(rt)), kind)


# --------------------------------------------------------------------------
# 2. kind = SGD is rfm_mf_sgd_levels_ex, and never reads the accumulators
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ms.step_cases()))
def test_sgd_kind_gives_the_bits_of_levels_ex(rt, name):
    case = ms.step_cases()[name]
    sched = ms.reach(case)
    init = case.init()
    want = ms.run_levels_ex(rt, case, sched, init)
    blank = []
    for a in init:
        s = np.empty(np.shape(a), dtype=np.float64)
        s.view(np.uint64)[...] = ms.SENTINEL_BITS
        blank.append(s)
    got = ma.run_levels_opt(rt, case, sched, init, blank, kind=ma.SGD, eps=float("nan"))
    _same_bits(got[:4], want, f"{name}: kind = SGD against rfm_mf_sgd_levels_ex")
    for a in got[4:]:
        assert (_bits(a) == ms.SENTINEL_BITS).all(), f"{name}: kind = SGD wrote an accumulator"
    # null accumulators are not looked at either
    state = ma.DeviceState(rt, init, blank)
    from relevance_factorizationmachine_amd import _lib
    _lib.check(ma.call_opt(rt, case.k, sched, ma.upload_schedule(rt, sched), state, ma.SGD, acc_ptrs=(None,) * 4))
    _same_bits(state.host()[:4], want, f"{name}: kind = SGD with null accumulators")


# --------------------------------------------------------------------------
# 3. edges of the rule and of the call
# --------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ma.ACC_KINDS)
@pytest.mark.parametrize("name", ["ring-cached-k16", "shape-k400"])
def test_learning_rate_zero_moves_the_accumulators_only(rt, name, kind):
    case = ms.step_cases()[name]
    sched = ms.reach(case)
    start = case.init() + ma.acc_init(case, kind)
    got = ma.run_levels_opt(rt, case, sched, start[:4], start[4:], lr=0.0)
    _same_bits(got[:4], start[:4], f"{name} {kind}: lr = 0")
    want = ma.oracle_of(case, kind, lr=0.0)
    ma.assert_all_within(got, want, start, case.pairs, f"{name} {kind} lr = 0")
    assert all((g >= s).all() and (g > s).any() for g, s in zip(got[4:], start[4:]))


@pytest.mark.parametrize("name", ["shape-k16", "ring-cached-k300"])
def test_an_accumulator_at_infinity_freezes_its_element(rt, name):
    case = ms.step_cases()[name]
    sched = ms.reach(case)
    start = [np.array(a) for a in case.init() + ma.acc_init(case, "uniform")]
    u, i = int(case.users[-1]), int(case.items[-1])  # (an item of the chains: cached)
    start[4][u, 0] = start[5][i, case.k - 1] = start[6][u] = start[7][i] = np.inf
    got = ma.run_levels_opt(rt, case, sched, start[:4], start[4:])
    for j, at in ((0, (u, 0)), (1, (i, case.k - 1)), (2, (u,)), (3, (i,))):
        assert _bits(got[j])[at] == _bits(start[j])[at], f"{name}: {ma.NAMES[j]} moved under G = +Inf"
        assert got[j + 4][at] == np.inf
    assert all(np.isfinite(g).sum() == g.size - (1 if j >= 4 else 0) for j, g in enumerate(got))
    # every other element of those rows moved as usual
    assert (got[0][u, 1:] != start[0][u, 1:]).all() and (got[1][i, :-1] != start[1][i, :-1]).all()


@pytest.mark.parametrize("kind", ma.ACC_KINDS)
@pytest.mark.parametrize("k", [1, 16, 400, 1023])
def test_a_batch_of_one_example(rt, k, kind):
    case = ms.Case(f"one-k{k}", k, np.array([1]), np.array([2]), {"levels_ex": [("seq", 0, 1)]})
    _check(rt, case, kind)


def _untouched_after(rt, case, start, what, **call):
    from relevance_factorizationmachine_amd import _lib
    sched = ms.reach(case)
    state = ma.DeviceState(rt, start[:4], start[4:])
    rc = ma.call_opt(rt, case.k, sched, ma.upload_schedule(rt, sched), state, **call)
    _same_bits(state.host(), start, what)
    return rc, _lib


def test_no_levels_no_launch(rt):
    case = ms.step_cases()["ring-cached-k16"]
    start = case.init() + ma.acc_init(case, "uniform")
    rc, _lib = _untouched_after(rt, case, start, "n_levels = 0", kind=ma.ADAGRAD, n_levels=0)
    assert rc == _lib.RFM_OK


def test_bad_arguments_leave_every_array_untouched(rt):
    case = ms.step_cases()["ring-cached-k16"]
    start = case.init() + ma.acc_init(case, "uniform")
    probe = ma.DeviceState(rt, start[:4], start[4:])
    accs = probe.accs.ptrs()
    calls = [dict(kind=2), dict(kind=-1)]
    calls += [dict(kind=ma.ADAGRAD, acc_ptrs=accs[:j] + (None,) + accs[j + 1:]) for j in range(4)]
    calls += [dict(kind=ma.ADAGRAD, eps=e) for e in (0.0, -1.0, float("nan"))]
    for call in calls:
        rc, _lib = _untouched_after(rt, case, start, f"bad argument {call}", **call)
        assert rc == _lib.RFM_ERR_BAD_ARG, call
    _same_bits(probe.host(), start, "the accumulators a refused call named")


# --------------------------------------------------------------------------
# 4. three batches in a row on the same arrays
# --------------------------------------------------------------------------
@pytest.mark.parametrize("k", [16, 400])
def test_three_batches_in_a_row(rt, k):
    """Each batch's oracle starts from the device's state before it (float64, so exact in long
    double): the tolerance of one batch then holds for each, and the accumulators carry over."""
    from relevance_factorizationmachine_amd import _lib
    from relevance_factorizationmachine_amd.runtime import mf_schedule_ex
    cases = [ms.step_cases()[f"ring-{kind}-k{k}"] for kind in ("cached", "start", "fresh")]
    nu, ni = max(c.n_users for c in cases), max(c.n_items for c in cases)
    state8 = tuple(cpu_ref.mf_init(ms.INIT_SEED, nu, ni, k))
    state8 = state8 + tuple(np.zeros(np.shape(a)) for a in state8)
    state = ma.DeviceState(rt, state8[:4], state8[4:])
    for case in cases:
        y, p = case.ry()
        sched = mf_schedule_ex(case.users, case.items, y, p, nu, ni, ms.capacity(k))
        assert ms.launch_plan(sched[1], k, "levels_ex") == case.want_plan["levels_ex"]
        want = ma.mf_adagrad_batch_ld(case.pairs, y / p, state8[:4], state8[4:], ms.B0, ms.LR, ms.REG, ma.EPS)
        _lib.check(ma.call_opt(rt, k, sched, ma.upload_schedule(rt, sched), state, ma.ADAGRAD))
        got = state.host()
        worst = ma.assert_all_within(got, want, state8, case.pairs, f"{case.name} in a row")
        print(f"distance {case.name} in a row parameters {worst[0]:.3e} accumulators {worst[1]:.3e}")
        state8 = got
    assert all((a > 0).any() for a in state8[4:])


# --------------------------------------------------------------------------
# 5. through Python
# --------------------------------------------------------------------------
def _model(est, g, **kw):
    import relevance_factorizationmachine_amd as pkg
    sh = synth.SHAPES["kuairec_small"]
    train, val = synth.make_log(sh, "MF", est, seed=0)
    args = dict(estimator=est, n_epochs=int(g["n_epochs"]), n_factors=int(g["n_factors"]), n_users=sh.n_users,
                n_items=sh.n_items, lr=float(g["lr"]), reg=float(g["reg"]), batch_size=int(g["batch_size"]),
                seed=int(g["seed"]))
    args.update(kw)
    m = pkg.LogisticMatrixFactorization(**args)
    m.optimizer, m.adagrad_eps, m.adagrad_init = "adagrad", float(g["eps"]), float(g["init"])
    return m, train, val


def _state(m):
    hs = (m.P, m.Q, m.b_u, m.b_i)
    return [h() for h in hs] + [h.acc.cpu().numpy() for h in hs]


@pytest.mark.parametrize("est", ["IPS", "Naive"])
def test_fit_against_the_reference_with_an_adagrad_subclass(est):
    import relevance_factorizationmachine_amd as pkg
    g = load_golden(GOLDEN[est])
    m, train, val = _model(est, g)
    tr, va = m.fit(train, val)
    assert all(isinstance(h, pkg.DeviceAdaGrad) for h in (m.P, m.Q, m.b_u, m.b_i))
    assert m.b == float(g[f"{est}_b"])
    names = ("P", "Q", "b_u", "b_i", "acc_P", "acc_Q", "acc_b_u", "acc_b_i")
    got = dict(zip(names, _state(m)), train_loss=tr, val_loss=va)
    for name, have in got.items():
        want = g[f"{est}_{name}"]
        print(f"{est} {name}: rel_err {rel_err(have, want):.3g}")
        assert rel_err(have, want) < TIGHT, name
        assert_elementwise(have, want, what=f"{est} {name}")


def test_fit_with_an_evaluator_leaves_the_same_parameters():
    from test_gpu_eval import _ValEvaluatorLike
    g = load_golden(GOLDEN["IPS"])
    states = []
    for with_ev in (False, True):
        ev = None
        if with_ev:
            _, val = synth.make_log(synth.SHAPES["kuairec_small"], "MF", "IPS", seed=0)
            ev = _ValEvaluatorLike(synth.interaction_frame(val, val["features"]), {"MF": val["features"]})
        m, train, val = _model("IPS", g, n_epochs=3, evaluator=ev)
        m.fit(train, val)
        if with_ev:
            assert len(m.val_metrics) == 3
        states.append(_state(m))
    _same_bits(states[1], states[0], "a fit with a ValEvaluator")
    assert all((a > 0).any() for a in states[0][4:])


def test_accumulators_persist_append_and_errors():
    import torch
    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import dist, mf
    g = load_golden(GOLDEN["IPS"])
    m, train, val = _model("IPS", g, n_epochs=2)
    m.adagrad_init = 0.25
    m.fit(train, val)
    acc1 = [a.copy() for a in _state(m)[4:]]
    assert all(a.min() >= 0.25 and a.max() > 0.25 for a in acc1)
    m.fit(train, val)  # the same handles: the accumulators go on growing
    acc2 = _state(m)[4:]
    assert all((b >= a).all() and (b > a).any() for a, b in zip(acc1, acc2))
    # append_users grows all four user-side tensors, the accumulators by adagrad_init
    rt, nu, k = m._rt, m.n_users, m.n_factors
    folded = mf.FoldedRows("user", torch.ones((3, k), dtype=torch.float64, device=rt.torch_device),
                           torch.ones(3, dtype=torch.float64, device=rt.torch_device), rt)
    assert list(m.append_users(folded)) == [nu, nu + 1, nu + 2] and m.n_users == nu + 3
    assert tuple(m.P.dev.shape) == tuple(m.P.acc.shape) == (nu + 3, k)
    assert tuple(m.b_u.dev.shape) == tuple(m.b_u.acc.shape) == (nu + 3,)
    assert np.array_equal(m.P.acc.cpu().numpy()[nu:], np.full((3, k), 0.25))
    assert np.array_equal(m.b_u.acc.cpu().numpy()[nu:], np.full(3, 0.25))
    assert np.array_equal(m.P.acc.cpu().numpy()[:nu], acc2[0]) and np.array_equal(m.b_u.acc.cpu().numpy()[:nu], acc2[2])
    assert tuple(m.Q.acc.shape) == (m.n_items, k)  # the item side is as it was
    m.fit(train, val)  # ... and the grown model fits on
    # not served with "adagrad": each a ValueError before any launch
    for make_bad, call, match in (
            (lambda b: setattr(b, "hogwild", True), lambda b, t, v: b.fit(t, v), "exact mode only"),
            (lambda b: None, lambda b, t, v: mf.fit_many([b], t, v), "SGD rule only"),
            (lambda b: None, lambda b, t, v: dist.hip_mf_partition_worker(b._rt, b, t, 1, 0), "SGD rule only"),
            (lambda b: setattr(b, "optimizer", "adam"), lambda b, t, v: b.fit(t, v), "optimizer must be"),
            (lambda b: setattr(b, "adagrad_eps", 0.0), lambda b, t, v: b.fit(t, v), "adagrad_eps")):
        bad, train, val = _model("IPS", g, n_epochs=2)
        make_bad(bad)
        before = [h() for h in (bad.P, bad.Q, bad.b_u, bad.b_i)]
        with pytest.raises(ValueError, match=match):
            call(bad, train, val)
        assert all(np.array_equal(a, h()) for a, h in zip(before, (bad.P, bad.Q, bad.b_u, bad.b_i)))
        assert type(bad.P) is pkg.DeviceSGD  # no handle changed its rule on the way to the error


@pytest.mark.parametrize("est", ["IPS", "Naive"])
def test_sgd_model_is_the_unchanged_path(est, monkeypatch):
    """``optimizer = "sgd"`` (the default) still equals mf_small.npz, through rfm_mf_sgd_levels_ex
    alone."""
    import relevance_factorizationmachine_amd as pkg
    g = load_golden("mf_small")
    sh = synth.SHAPES["kuairec_small"]
    train, val = synth.make_log(sh, "MF", est, seed=0)
    m = pkg.LogisticMatrixFactorization(estimator=est, n_epochs=3, n_factors=16, n_users=sh.n_users,
                                        n_items=sh.n_items, lr=0.01, reg=0.5, batch_size=2000, seed=12345)
    assert m.optimizer == "sgd"
    calls = {"ex": 0, "opt": 0}
    lib = m._rt.lib
    real_ex, real_opt = lib.rfm_mf_sgd_levels_ex, lib.rfm_mf_sgd_levels_opt

    def counted(name, real):
        def call(*args):
            calls[name] += 1
            return real(*args)
        return call

    monkeypatch.setattr(lib, "rfm_mf_sgd_levels_ex", counted("ex", real_ex), raising=False)
    monkeypatch.setattr(lib, "rfm_mf_sgd_levels_opt", counted("opt", real_opt), raising=False)
    tr, va = m.fit(train, val)
    assert calls == {"ex": 3, "opt": 0}
    assert type(m.P) is pkg.DeviceSGD and not hasattr(m.P, "acc")
    for got, name in ((m.P(), "P"), (m.Q(), "Q"), (m.b_u(), "b_u"), (m.b_i(), "b_i"), (tr, "train_loss"),
                      (va, "val_loss")):
        assert rel_err(got, g[f"{est}_{name}"]) < TIGHT, name
        assert_elementwise(got, g[f"{est}_{name}"], what=f"mf_small {est} {name}")
