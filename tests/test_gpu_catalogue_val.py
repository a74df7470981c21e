"""Catalogue metrics per iteration inside ``fit()``: ``rfm_rank_metrics`` and
``rfm_pair_ranks_n`` through the C ABI, ``evaluate.CatalogueValEvaluator`` one-shot on the fixture
models and as ``evaluator=`` of ``FactorizationMachines`` / ``LogisticMatrixFactorization``.  Needs
an MI355X: ``pytest -m gpu``.  Metric values are held to the catalogue metrics' own tolerance,
1e-12 relative (``rank_items_common.assert_metrics_equal``); everything the device computes twice is
compared bit for bit."""
import numpy as np
import pytest
from scipy import sparse as sp

import catalogue_val_common as cv
import rank_items_common as rk
import recommend_common as rc
import test_gpu_rank_items as tri
import test_gpu_recommend as tgr
from conftest import load_golden
from oracle import cpu_ref
from relevance_factorizationmachine_amd.evaluate import CatalogueEvaluator, CatalogueValEvaluator

pytestmark = pytest.mark.gpu

NU, NI = rc.N_USERS, rc.N_ITEMS
RTOL = 1e-12


@pytest.fixture(scope="module")
def rfm():
    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import features, recommend, runtime
    return pkg, features, recommend, runtime.Runtime.get()


@pytest.fixture(scope="module")
def gold():
    return load_golden("recommend"), {layout: load_golden(f"recommend_fm_{layout}") for layout in rc.LAYOUTS}


@pytest.fixture(scope="module")
def held(gold):
    """``(train mask, positives, exclusion lists)`` of the fixture's held-out split."""
    train, positives, _ = rk.heldout(gold[0])
    return train, positives, sp.csr_matrix(train.astype(np.float64))


# --------------------------------------------------------------------------- 1
def _abi_metrics(rfm, indptr, ranks, cand, weights, K, raw=None):
    """``(out [3 n_K + 2], counts [3], workspace bytes)`` of one ``rfm_rank_metrics`` call."""
    import ctypes as C

    import torch
    from relevance_factorizationmachine_amd import _lib
    rt = rfm[3]
    n_sel, n_tgt = indptr.shape[0] - 1, ranks.shape[0]
    nbytes = C.c_int64(0)
    _lib.check(rt.lib.rfm_rank_metrics_workspace(n_sel, n_tgt, len(K), C.byref(nbytes)))
    ws = rt.empty((nbytes.value,), torch.uint8)
    out = torch.full((3 * len(K) + 2,), 7.0, dtype=torch.float64, device=rt.torch_device)
    counts = torch.full((3,), -7, dtype=torch.int64, device=rt.torch_device)
    d_indptr, d_ranks = rt.upload(indptr), rt.upload(ranks if n_tgt else np.zeros(1, np.int32))
    d_cand = rt.upload(cand if n_sel else np.zeros(1, np.int32))
    d_w = None if weights is None else rt.upload(weights if n_tgt else np.zeros(1))
    h_K = np.ascontiguousarray(K, dtype=np.int64)
    args = dict(ctx=rt.ctx, indptr=d_indptr.data_ptr(), n_sel=n_sel, n_tgt=n_tgt, ranks=d_ranks.data_ptr(),
                cand=d_cand.data_ptr(), w=None if d_w is None else d_w.data_ptr(), K=h_K.ctypes.data, n_K=len(K),
                ws=ws.data_ptr(), out=out.data_ptr(), counts=counts.data_ptr())
    args.update(raw or {})
    _lib.check(rt.lib.rfm_rank_metrics(*args.values()))
    rt.sync()
    return out.cpu().numpy(), counts.cpu().numpy(), nbytes.value


def _as_metrics(out, n_K):
    return {"DCG": out[:n_K], "Recall": out[n_K:2 * n_K], "MAP": out[2 * n_K:3 * n_K], "MRR": out[3 * n_K:3 * n_K + 1],
            "AUC": out[3 * n_K + 1:]}


@pytest.mark.parametrize("rank0", ["mixed", "present", "absent"])
@pytest.mark.parametrize("n_users", [1, 64, 65, 130])
def test_rank_metrics_against_the_host_statement(rfm, n_users, rank0):
    K = cv.ABI_K
    indptr, ranks, cand, weights = cv.synthetic_ranks(n_users, seed=n_users + 3 * len(rank0), rank0=rank0)
    has0 = [0 in ranks[indptr[s]:indptr[s + 1]] for s in range(n_users)]
    if rank0 == "absent":  # (the last of several users has C == P: every rank)
        assert not any(has0[:-1] if n_users > 1 else has0)
    if rank0 == "present":
        assert any(has0)
    want, wdcg, counts = cv.host_answer(indptr, ranks, cand, weights, K)
    if n_users > 1:  # a user with no ranked positive, a user with C == P, some positives unranked
        assert counts[0] <= n_users - 1 and counts[1] <= counts[0] - 1 and counts[2] > 0
    out, got_counts, _ = _abi_metrics(rfm, indptr, ranks, cand, None, K)
    rk.assert_metrics_equal(_as_metrics(out, len(K)), want, f"{n_users} users, rank 0 {rank0}", rtol=RTOL)
    assert tuple(int(c) for c in got_counts) == counts
    # weights enter the DCG and nothing else
    out_w, counts_w, _ = _abi_metrics(rfm, indptr, ranks, cand, weights, K)
    print("weighted DCG", out_w[:len(K)], wdcg)
    assert np.all(np.abs(out_w[:len(K)] - wdcg) <= RTOL * np.abs(wdcg))
    assert out_w[len(K):].tobytes() == out[len(K):].tobytes() and counts_w.tobytes() == got_counts.tobytes()
    # the same inputs, the same bytes
    again, counts_again, _ = _abi_metrics(rfm, indptr, ranks, cand, weights, K)
    assert again.tobytes() == out_w.tobytes() and counts_again.tobytes() == counts_w.tobytes()
    # the order in which a user's targets are listed does not matter: the sums go by rank
    perm = np.concatenate([indptr[s] + np.random.default_rng(s).permutation(indptr[s + 1] - indptr[s])
                           for s in range(n_users)])
    shuffled, _, _ = _abi_metrics(rfm, indptr, ranks[perm], cand, weights[perm], K)
    assert shuffled.tobytes() == out_w.tobytes()


def test_rank_metrics_with_every_user_dropped(rfm):
    K = cv.ABI_K
    indptr, ranks, cand, weights = cv.synthetic_ranks(65, seed=5, all_dropped=True)
    out, counts, _ = _abi_metrics(rfm, indptr, ranks, cand, weights, K)
    assert np.isnan(out).all() and out.shape == (3 * len(K) + 2,)
    assert counts.tolist() == [0, 0, int(ranks.shape[0])]
    # users without a target, and no user at all
    out, counts, _ = _abi_metrics(rfm, np.zeros(4, np.int64), np.zeros(0, np.int32), np.full(3, 9, np.int32), None, K)
    assert np.isnan(out).all() and counts.tolist() == [0, 0, 0]
    out, counts, _ = _abi_metrics(rfm, np.zeros(1, np.int64), np.zeros(0, np.int32), np.zeros(0, np.int32), None, [3])
    assert np.isnan(out).all() and out.shape == (5,) and counts.tolist() == [0, 0, 0]


def test_rank_metrics_small_case_by_hand(rfm):
    """Two users: ranks {0, 2} of 5 candidates, and rank {3} of 4."""
    indptr, ranks = np.array([0, 2, 3], np.int64), np.array([2, 0, 3], np.int32)
    out, counts, _ = _abi_metrics(rfm, indptr, ranks, np.array([5, 4], np.int32), np.array([2.0, 4.0, 8.0]), [1, 3, 4])
    got = _as_metrics(out, 3)
    g2, g3 = 1.0 / np.log2(3.0), 1.0 / np.log2(4.0)
    np.testing.assert_allclose(got["DCG"], [(4.0 + 0.0) / 2, (4.0 + 2.0 * g2) / 2, (4.0 + 2.0 * g2 + 8.0 * g3) / 2], rtol=RTOL)
    np.testing.assert_allclose(got["Recall"], [0.25, 0.5, 1.0], rtol=RTOL)
    np.testing.assert_allclose(got["MAP"], [0.5, (1.0 + 2.0 / 3.0) / 2, (1.0 + 2.0 / 3.0 + 0.25) / 2], rtol=RTOL)
    np.testing.assert_allclose(got["MRR"], [(1.0 + 0.25) / 2], rtol=RTOL)
    np.testing.assert_allclose(got["AUC"], [((1.0 - 1.0 / 6.0) + 0.0) / 2], rtol=RTOL)
    assert counts.tolist() == [2, 2, 0]


def test_rank_metrics_rejects_bad_arguments(rfm, monkeypatch):
    indptr, ranks, cand = np.array([0, 2, 3], np.int64), np.array([2, 0, 3], np.int32), np.array([5, 4], np.int32)
    for raw, match in (({"n_K": 0}, "n_K"), ({"n_K": 17}, "n_K"), ({"ws": None}, "null"), ({"out": None}, "null"),
                       ({"counts": None}, "null"), ({"K": None}, "null"), ({"indptr": None}, "null"),
                       ({"ranks": None}, "null"), ({"n_sel": -1}, "n_sel_users"), ({"n_tgt": -1}, "n_targets")):
        with pytest.raises(ValueError, match=match):
            _abi_metrics(rfm, indptr, ranks, cand, None, [1, 3], raw=raw)
    with pytest.raises(ValueError, match="depth"):
        _abi_metrics(rfm, indptr, ranks, cand, None, [1, 0])
    # an indptr that does not end at n_targets: clamped (never followed outside the arrays), and an
    # error under RFM_CHECK_IDS=1
    _abi_metrics(rfm, np.array([0, 2, 9], np.int64), ranks, cand, None, [1, 3])
    monkeypatch.setenv("RFM_CHECK_IDS", "1")
    _abi_metrics(rfm, indptr, ranks, cand, None, [1, 3])
    with pytest.raises(ValueError, match="target indptr"):
        _abi_metrics(rfm, np.array([0, 2, 9], np.int64), ranks, cand, None, [1, 3])


# --------------------------------------------------------------------------- 2
def _abi_ranks_n(rfm, A, LU, B, LI, c, tgt_indptr, tgt_items, user_ids=None, excl=None):
    """``tri._abi_ranks`` through ``rfm_pair_ranks_n``: the target count comes from the host."""
    _, _, recommend, rt = rfm
    import torch
    from relevance_factorizationmachine_amd import _lib
    kf = A.shape[1]
    dA, dB = recommend.padded(rt, rt.upload(A), kf), recommend.padded(rt, rt.upload(B), kf)
    dLU, dLI, dc = rt.upload(LU), rt.upload(LI), rt.upload(np.array([c], dtype=np.float64))
    ids = None if user_ids is None else rt.upload(np.asarray(user_ids, dtype=np.int32))
    n_sel = A.shape[0] if user_ids is None else len(user_ids)
    tgt_indptr, tgt_items = np.asarray(tgt_indptr, dtype=np.int64), np.asarray(tgt_items, dtype=np.int32)
    n_tgt = int(tgt_items.shape[0])
    d_indptr = rt.upload(tgt_indptr)
    d_items = rt.upload(tgt_items) if n_tgt else None
    ws = rt.empty((recommend.ranks_workspace_bytes(n_sel, B.shape[0], n_tgt),), torch.uint8)
    ranks, scores = rt.empty((max(n_tgt, 1),), torch.int32), rt.empty((max(n_tgt, 1),), torch.float64)
    cand = rt.empty((max(n_sel, 1),), torch.int32)
    ex = (None, None) if excl is None else (rt.upload(excl[0].astype(np.int64)), rt.upload(excl[1].astype(np.int32)))
    ptr = lambda t: None if t is None else t.data_ptr()  # noqa: E731
    _lib.check(rt.lib.rfm_pair_ranks_n(
        rt.ctx, dA.data_ptr(), dLU.data_ptr(), A.shape[0], ptr(ids), n_sel, dB.data_ptr(), dLI.data_ptr(), B.shape[0],
        kf, dc.data_ptr(), ptr(ex[0]), ptr(ex[1]), d_indptr.data_ptr(), ptr(d_items), n_tgt,
        ws.data_ptr() if n_tgt else None, ranks.data_ptr() if n_tgt else None, scores.data_ptr() if n_tgt else None,
        cand.data_ptr()))
    rt.sync()
    return ranks.cpu().numpy()[:n_tgt], scores.cpu().numpy()[:n_tgt], cand.cpu().numpy()[:n_sel]


@pytest.mark.parametrize("n_users,n_items,kf", [(70, 150, 6), (3, 5, 4)])
def test_pair_ranks_n_gives_the_bytes_of_pair_ranks(rfm, n_users, n_items, kf):
    rng, A, LU, B, LI, c, logit = tri._order_rule_operands(n_users, n_items, kf)
    indptr, tgt = np.arange(n_users + 1) * n_items, np.tile(np.arange(n_items), n_users)  # all pairs
    M = rng.random((n_users, n_items)) < 0.3
    E = sp.csr_matrix(M.astype(np.float64))
    sel = rng.integers(0, n_users, size=n_users + 7)
    counts = rng.integers(0, 2 * n_items, size=sel.shape[0])
    counts[0] = 0
    indptr2 = np.concatenate(([0], np.cumsum(counts)))
    tgt2 = np.concatenate([np.sort(rng.integers(0, n_items, size=n)) for n in counts])
    for what, args, kw in (("all pairs", (indptr, tgt), {}),
                           ("exclusion lists", (indptr, tgt), {"excl": (E.indptr, E.indices)}),
                           ("permuted users", (indptr2, tgt2), {"user_ids": sel, "excl": (E.indptr, E.indices)}),
                           ("no targets", (np.zeros(n_users + 1, np.int64), np.zeros(0, np.int32)), {})):
        want = tri._abi_ranks(rfm, A, LU, B, LI, c, *args, **kw)
        got = _abi_ranks_n(rfm, A, LU, B, LI, c, *args, **kw)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), what
    np.testing.assert_array_equal(got[2], n_items - 1)  # no targets: the candidates are still counted


# --------------------------------------------------------------------------- 3
def _model(rfm, gold, model):
    if model[0] == "mf":
        return tgr._mf_model(rfm[0], gold[0], model[2]), None
    m, sides, _, _ = tgr._fixture_model(rfm, gold, *model[1:])
    return m, sides


@pytest.mark.parametrize("model", rk.MODELS, ids=rk.model_id)
def test_one_shot_evaluation_of_the_fixture_models(rfm, gold, held, model):
    train, positives, E = held
    m, sides = _model(rfm, gold, model)
    Z = rk.model_logits(gold[0], gold[1], model)
    assert rk.min_relative_gap(Z) >= 4e-9  # the ranks, hence the comparisons below, are not a coin toss
    rng = np.random.default_rng(7)
    pscores = rng.uniform(0.05, 1.0, size=positives[0].shape[0])
    ev = CatalogueValEvaluator(positives, NI, rk.K_LIST, rk.METRICS, ("DCG", 5), sides=sides, exclude=E, pscores=pscores)
    got = ev.evaluate(m)  # "Naive"
    assert ev.unranked == 0 and list(got) == rk.METRICS
    rk.assert_metrics_equal(got, CatalogueEvaluator(positives, NI, rk.K_LIST, rk.METRICS, exclude=E).evaluate(m, sides),
                            rk.model_id(model) + " vs CatalogueEvaluator", rtol=RTOL)
    rk.assert_metrics_equal(got, rk.oracle_metrics(Z, positives, train), rk.model_id(model) + " vs oracle", rtol=RTOL)
    # IPS: DCG@K is the reference's ValEvaluator metric on the frame of all candidate pairs of the
    # users with a positive; every other metric has no weighted form
    ips = ev.evaluate(m, estimator="IPS")
    label, ps = np.zeros(Z.shape), np.ones(Z.shape)
    label[positives] = 1.0
    ps[positives] = pscores
    fu, fi = np.nonzero(~train & ~np.isnan(Z) & np.isin(np.arange(NU), positives[0])[:, None])
    frame = {"user": fu, "label": label[fu, fi], "pscore": ps[fu, fi], "ones_pscore": np.ones(fu.shape[0])}
    want = np.array([cpu_ref.val_dcg(frame, Z[fu, fi], "IPS", k=k) for k in rk.K_LIST])
    print("IPS DCG", ips["DCG"], want)
    assert np.all(np.abs(np.asarray(ips["DCG"]) - want) <= RTOL * np.abs(want))
    naive = np.array([cpu_ref.val_dcg(frame, Z[fu, fi], "Naive", k=k) for k in rk.K_LIST])
    assert np.all(np.abs(np.asarray(got["DCG"]) - naive) <= RTOL * np.abs(naive))
    assert not np.allclose(ips["DCG"], got["DCG"])
    for name in ("Recall", "MAP", "MRR", "AUC"):
        assert ips[name] == got[name]
    cv.assert_same_bits(ev.evaluate(m, "Naive"), got, "evaluated twice")
    # without pscores the estimator changes nothing; without exclusion lists the train pairs compete
    plain = CatalogueValEvaluator(positives, NI, rk.K_LIST, rk.METRICS, ("MRR", None), sides=sides)
    cv.assert_same_bits(plain.evaluate(m, "IPS"), plain.evaluate(m), "no pscores")
    rk.assert_metrics_equal(plain.evaluate(m), rk.oracle_metrics(Z, positives, np.zeros_like(train)),
                            rk.model_id(model) + " no exclusion", rtol=RTOL)


# --------------------------------------------------------------------------- 4, 5, 7
FM_CURVES = {  # (layout, k, alpha): compare with the oracle's refits too (d)?
    ("kuairec", 16, 2.0): False,   # neighbouring logits fall to 7.3e-9 apart during these iterations: (b) only
    ("kuairec", 400, 0.25): True,  # the sliced forwards; smallest relative gap over the 8 iterations 1.66e-8
    ("coat", 16, 2.0): True,       # 1.96e-8
}
_cache = {}


def _sides(rfm, gold, layout):
    if layout not in _cache:
        _cache[layout] = tgr._sides(rfm, gold[0], layout)
    return _cache[layout]


def _fm(rfm, gold, case, n_epochs, evaluator=None, lr=None):
    layout, k, alpha = case
    g, gl = gold[0], gold[1][layout]
    m = rfm[0].FactorizationMachines(
        estimator="IPS", n_epochs=n_epochs, n_factors=k, n_features=_sides(rfm, gold, layout).n_features,
        lr=float(gl[f"{rc.case_name(k, alpha)}_lr"]) if lr is None else lr, batch_size=int(g["batch_size"]),
        seed=int(g["seed"]), alpha=alpha, evaluator=evaluator)
    m.deterministic = True
    return m


def _fm_evaluator(rfm, gold, held, case, monitor=("DCG", 5), every=1):
    """The weighted form rides along on the case that is not compared with the unweighted oracle."""
    _, positives, E = held
    pscores = None if FM_CURVES[case] else np.random.default_rng(11).uniform(0.05, 1.0, size=positives[0].shape[0])
    return CatalogueValEvaluator(positives, NI, rk.K_LIST, rk.METRICS, monitor, sides=_sides(rfm, gold, case[0]),
                                 exclude=E, pscores=pscores, every=every)


def _fm_curve(rfm, gold, held, case):
    """One fit of ``cv.N_ITERS`` iterations with the evaluator, shared by the tests below."""
    if case not in _cache:
        split = cv.fixture_split(gold[0], case[0])
        ev = _fm_evaluator(rfm, gold, held, case)
        m = _fm(rfm, gold, case, cv.N_ITERS, ev)
        tl, vl = m.fit(*split)
        _cache[case] = (split, ev, m, tl, vl)
    return _cache[case]


def _bits(*arrays):
    return [np.asarray(a, dtype=np.float64).tobytes() for a in arrays]


@pytest.mark.parametrize("case", list(FM_CURVES), ids=lambda c: f"{c[0]}-{rc.case_name(c[1], c[2])}")
def test_fm_curve_inside_fit(rfm, gold, held, case):
    train_mask, positives, _ = held
    split, ev, m, tl, vl = _fm_curve(rfm, gold, held, case)
    assert (m.plan_info["slices"] > 0) == (case[1] > 128)  # k = 400 trains with the sliced forwards
    # (a) training is what it is without an evaluator
    bare = _fm(rfm, gold, case, cv.N_ITERS)
    tl0, vl0 = bare.fit(*split)
    assert _bits(tl, vl, m.w0(), m.w(), m.V()) == _bits(tl0, vl0, bare.w0(), bare.w(), bare.V())
    assert not hasattr(bare, "val_metrics")
    # (c) val_metrics is the monitored column
    assert len(m.val_metrics) == cv.N_ITERS and all(isinstance(v, float) for v in m.val_metrics)
    assert _bits(m.val_metrics) == _bits(ev.history["DCG"][:, rk.K_LIST.index(5)])
    assert {k: v.shape for k, v in ev.history.items()} == {
        name: (cv.N_ITERS, 1 if name in ("MRR", "AUC") else len(rk.K_LIST)) for name in rk.METRICS}
    assert ev.unranked_history.dtype == np.int64 and ev.unranked_history.tolist() == [0] * cv.N_ITERS
    assert int(np.argmax(m.val_metrics)) == int(np.argmax(ev.history["DCG"][:, rk.K_LIST.index(5)]))
    # (b) row e is the one-shot evaluation of a fresh model fitted for e + 1 iterations
    one_shot = _fm_evaluator(rfm, gold, held, case)
    XU, XI = rc.side_matrices(case[0], gold[0]["user_table"], gold[0]["item_table"], gold[0]["context"])
    lr = float(gold[1][case[0]][f"{rc.case_name(case[1], case[2])}_lr"])
    for e in range(cv.N_ITERS):
        fresh = _fm(rfm, gold, case, e + 1)
        fresh.fit(*split)
        cv.assert_same_bits(cv.row(ev.history, e), one_shot.evaluate(fresh, estimator="IPS"), f"iteration {e}")
        if FM_CURVES[case]:  # (d) and the oracle's refit says the same within the metrics' tolerance
            ref = cpu_ref.fm_fit(split[0], split[1], n_epochs=e + 1, n_factors=case[1], lr=lr,
                                 batch_size=int(gold[0]["batch_size"]), seed=int(gold[0]["seed"]), alpha=case[2],
                                 with_losses=False)
            Z = rc.fm_logits(XU, XI, ref["w0"], ref["w"], ref["V"])
            assert rk.min_relative_gap(Z) >= 1e-8  # ten times the fit's parity bound of 1e-9
            rk.assert_metrics_equal(cv.row(ev.history, e), rk.oracle_metrics(Z, positives, train_mask),
                                    f"iteration {e} vs oracle", rtol=RTOL)
    curve = ev.history["DCG"][:, rk.K_LIST.index(5)]
    assert np.unique(curve).shape[0] > 1  # not a constant: an off-by-one in the iteration would show


def test_every_third_iteration(rfm, gold, held):
    case = ("kuairec", 16, 2.0)
    split, ev1, m1, tl1, vl1 = _fm_curve(rfm, gold, held, case)
    ev = _fm_evaluator(rfm, gold, held, case, monitor=("Recall", 9), every=3)
    m = _fm(rfm, gold, case, cv.N_ITERS, ev)
    tl, vl = m.fit(*split)
    assert _bits(tl, vl, m.w0(), m.w(), m.V()) == _bits(tl1, vl1, m1.w0(), m1.w(), m1.V())
    for e in range(cv.N_ITERS):
        if e in (2, 5, 7):
            cv.assert_same_bits(cv.row(ev.history, e), cv.row(ev1.history, e), f"iteration {e}")
            assert ev.unranked_history[e] == 0
        else:
            assert all(np.isnan(v[e]).all() for v in ev.history.values()) and ev.unranked_history[e] == -1
    assert len(m.val_metrics) == cv.N_ITERS
    col = ev1.history["Recall"][:, rk.K_LIST.index(9)]
    assert _bits(np.asarray(m.val_metrics)[[2, 5, 7]]) == _bits(col[[2, 5, 7]])
    assert int(np.nanargmax(m.val_metrics)) == [2, 5, 7][int(np.argmax(col[[2, 5, 7]]))]


def test_a_fit_that_overflows_still_returns(rfm, gold, held):
    case = ("kuairec", 16, 2.0)
    split = cv.fixture_split(gold[0], case[0])
    ev = _fm_evaluator(rfm, gold, held, case, monitor=("MRR", None))
    m = _fm(rfm, gold, case, 4, ev, lr=1e200)
    tl, vl = m.fit(*split)
    assert len(tl) == len(vl) == len(m.val_metrics) == 4
    assert np.isnan(m.V()).any()
    n_pos = held[1][0].shape[0]
    # from the second iteration on every parameter is NaN: no positive has a rank, no user counts
    assert np.isnan(m.val_metrics[1:]).all()
    assert ev.unranked_history[1:].tolist() == [n_pos] * 3 and ev.unranked == n_pos
    assert all(np.isnan(v[1:]).all() for v in ev.history.values())
    first = ev.unranked_history[0]
    assert 0 <= first <= n_pos


def test_fit_refuses_sides_that_do_not_fit(rfm, gold, held):
    case = ("kuairec", 16, 2.0)
    split = cv.fixture_split(gold[0], case[0])
    _, positives, E = held
    ev = CatalogueValEvaluator(positives, NI, rk.K_LIST, rk.METRICS, ("DCG", 5), exclude=E)
    with pytest.raises(ValueError, match="needs sides"):
        _fm(rfm, gold, case, 2, ev).fit(*split)
    ev = CatalogueValEvaluator(positives, NI, rk.K_LIST, rk.METRICS, ("DCG", 5), sides=_sides(rfm, gold, "kuairec"))
    with pytest.raises(ValueError, match="takes no sides"):
        _mf(rfm, gold, 24, 2, ev).fit(*cv.fixture_split(gold[0]))


# --------------------------------------------------------------------------- 6
def _mf(rfm, gold, k, n_epochs, evaluator=None):
    g = gold[0]  # the hyper-parameters of tests/golden/make_golden_recommend.py
    return rfm[0].LogisticMatrixFactorization(
        estimator="IPS", n_epochs=n_epochs, n_factors=k, n_users=NU, n_items=NI, lr=0.02, reg=0.5,
        batch_size=int(g["batch_size"]), seed=int(g["seed"]), evaluator=evaluator)


@pytest.mark.parametrize("k", rc.MF_FACTORS)  # 33: n_factors % 4 != 0, the padded operands
def test_mf_curve_inside_fit(rfm, gold, held, k):
    """Both factor counts meet the precondition of the oracle comparison: over the 3 iterations the
    smallest relative gap between neighbouring logits of a user is 2.1e-7 (k = 24) and 6.3e-8
    (k = 33), checked on the CPU with ``cpu_ref.mf_fit``."""
    train_mask, positives, E = held
    g = gold[0]
    n_iters = int(g["mf_iters"])
    split = cv.fixture_split(g)
    pscores = np.random.default_rng(13).uniform(0.05, 1.0, size=positives[0].shape[0])
    make = lambda ps: CatalogueValEvaluator(positives, NI, rk.K_LIST, rk.METRICS, ("MAP", 9), exclude=E, pscores=ps)  # noqa: E731
    ev = make(None)
    m = _mf(rfm, gold, k, n_iters, ev)
    tl, vl = m.fit(*split)
    bare = _mf(rfm, gold, k, n_iters)
    tl0, vl0 = bare.fit(*split)
    assert _bits(tl, vl, m.P(), m.Q(), m.b_u(), m.b_i()) == _bits(tl0, vl0, bare.P(), bare.Q(), bare.b_u(), bare.b_i())
    assert len(m.val_metrics) == n_iters
    assert _bits(m.val_metrics) == _bits(ev.history["MAP"][:, rk.K_LIST.index(9)])
    assert ev.unranked_history.tolist() == [0] * n_iters
    one_shot = make(None)
    for e in range(n_iters):
        fresh = _mf(rfm, gold, k, e + 1)
        fresh.fit(*split)
        cv.assert_same_bits(cv.row(ev.history, e), one_shot.evaluate(fresh, estimator="IPS"), f"iteration {e}")
        ref = cpu_ref.mf_fit(split[0], split[1], n_epochs=e + 1, n_factors=k, lr=0.02, batch_size=int(g["batch_size"]),
                             seed=int(g["seed"]), n_users=NU, n_items=NI, reg=0.5)
        Z = rc.mf_logits(ref["P"], ref["Q"], ref["b_u"], ref["b_i"], ref["b"])
        assert rk.min_relative_gap(Z) >= 1e-8
        rk.assert_metrics_equal(cv.row(ev.history, e), rk.oracle_metrics(Z, positives, train_mask),
                                f"mf k={k} iteration {e} vs oracle", rtol=RTOL)
    # a second fit() on the same model goes on from its parameters and appends a second curve
    first = {name: v.copy() for name, v in ev.history.items()}
    first_curve = list(m.val_metrics)
    m.fit(*split)
    assert len(m.val_metrics) == 2 * n_iters and _bits(m.val_metrics[:n_iters]) == _bits(first_curve)
    assert _bits(m.val_metrics[n_iters:]) == _bits(ev.history["MAP"][:, rk.K_LIST.index(9)])
    assert _bits(m.val_metrics[n_iters:]) != _bits(first_curve)
    # with propensities and the IPS estimator the DCG columns are the weighted ones, the rest stays
    weighted = make(pscores)
    mw = _mf(rfm, gold, k, n_iters, weighted)
    mw.fit(*split)
    for name in ("Recall", "MAP", "MRR", "AUC"):
        assert _bits(weighted.history[name]) == _bits(first[name])
    assert not np.allclose(weighted.history["DCG"], first["DCG"])
    cv.assert_same_bits(cv.row(weighted.history, n_iters - 1), weighted.evaluate(mw, estimator="IPS"), "weighted, last row")
    cv.assert_same_bits(cv.row(first, n_iters - 1), weighted.evaluate(mw, estimator="Naive"), "unweighted, last row")


# --------------------------------------------------------------------------- 8
@pytest.mark.parametrize("kind,k", [("mf", 33), ("fm", 6)])
def test_operands_refreshed_in_place_are_fresh_operands(rfm, kind, k):
    """``recommend.operands(into=)``, what the evaluator does between iterations: after the
    parameters changed on the device, every tensor of the refreshed operands has the bytes of
    operands built anew -- the zero columns k .. kpad-1 included (MF k = 33: kpad = 36, the padded
    copies; FM k = 6: kpad = 8) -- in the memory the first call allocated.  65 users x 70 items:
    two tiles a side, the second partial."""
    pkg, _, recommend, rt = rfm
    nu, ni, kp = 65, 70, recommend.pad4(k)
    rng = np.random.default_rng(k)
    if kind == "fm":
        cu, ci = 9, 12  # user columns, then item columns: disjoint
        XU = sp.hstack([sp.random(nu, cu, 0.5, random_state=1, data_rvs=rng.standard_normal), sp.csr_matrix((nu, ci))])
        XI = sp.hstack([sp.csr_matrix((ni, cu)), sp.random(ni, ci, 0.5, random_state=2, data_rvs=rng.standard_normal)])
        sides = recommend.Sides(XU.tocsr(), XI.tocsr())
        model = tgr._fm_model(pkg, cu + ci, k, 2.0, 0.25, rng.standard_normal(cu + ci), rng.standard_normal((cu + ci, k)))
        params, owned = (model.w0, model.w, model.V), ("A", "LU", "B", "LI")
    else:
        sides = None
        model = pkg.LogisticMatrixFactorization(estimator="IPS", n_epochs=1, n_factors=k, n_users=nu, n_items=ni, lr=0.02,
                                                reg=0.5, batch_size=1, seed=12345)
        for p, shape in ((model.P, (nu, k)), (model.Q, (ni, k)), (model.b_u, nu), (model.b_i, ni)):
            p.set(rng.standard_normal(shape))
        model.b = 0.375
        params, owned = (model.P, model.Q, model.b_u, model.b_i), ("A", "B", "c")
    first = recommend.operands(model, sides)
    rt.sync()
    before = [t.cpu().numpy().copy() for t in first[1:6]]
    for p, scale in zip(params, (2.0, 0.5, 4.0, 0.25)):  # exact: powers of two
        p.dev.mul_(scale)
    if kind == "mf":
        model.b = 3.0
    again = recommend.operands(model, sides, into=first)
    fresh = recommend.operands(model, sides)
    rt.sync()
    assert again.A.shape == (nu, kp) and again.B.shape == (ni, kp) and kp > k
    for name, a, f, b in zip(("A", "LU", "B", "LI", "c"), again[1:6], fresh[1:6], before):
        a, f = a.cpu().numpy(), f.cpu().numpy()
        assert a.shape == f.shape and a.tobytes() == f.tobytes(), name
        assert a.tobytes() != b.tobytes(), (name, "the refresh changed nothing")
    for M in (again.A, again.B):
        assert not M.cpu().numpy()[:, k:].any()
    for name in owned:
        assert getattr(again, name).data_ptr() == getattr(first, name).data_ptr(), name
        assert getattr(fresh, name).data_ptr() != getattr(first, name).data_ptr(), name
    assert (again.rt, again.n_factors, again.n_users, again.n_items) == (rt, k, nu, ni)
