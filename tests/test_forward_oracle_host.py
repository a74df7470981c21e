"""The row oracle and the tolerances of forward_rows_common.py, checked on the CPU: the oracle
equals the float64 reference (oracle/cpu_ref.py) to float64 rounding, a float64 evaluation in a
shuffled order stays below half of each tolerance on every kind of input test_gpu_forward_rows.py
uses, at least 80 % of every input's rows are unsaturated, and the tolerances are sharp: each of
four mutations a kernel could make breaks them on the affected row and only there.  No GPU needed.

The device tests size their logs by the device (rows of a trip, of a pass); the inputs here are
the same generators' logs at HOST_ROWS rows, with the trip edges of a 256-thread workgroup."""
import numpy as np
import pytest

import forward_rows_common as fr
import grad_forms_common as gf
from oracle import cpu_ref

LD = np.longdouble
KS = sorted(gf.CLASS_OF)


def _inputs(k):
    """The kinds of log of test_gpu_forward_rows.py for a factor count: (name, log, theta, oracle)."""
    lpr = gf.CLASS_OF[k][0]
    g = 256 // lpr
    out = [("rows", *fr.case(k, fr.HOST_ROWS, (16 + g, 17 + 2 * g), ((19 + 4 * g, 19 + 5 * g),)))]
    out.append(("row blocks", *fr.case(k, fr.HOST_ROWS, (), (), lpr, 21, None, 8, 0)))
    out.append(("records", *fr.case(k, fr.HOST_ROWS, (), (), 2 * lpr + 1, 21, None, 8, 0)))
    return out


# (factor count, lanes per row) of the rfm_fm_train cases: a training log and a validation log each
TRAIN_CASES = [(16, 8), (32, 16), (128, 64), (130, 64), (200, 64), (300, 64), (600, 64)]


def _rows64(begin, length, cols, x, w0, w, V, rng=None):
    """Float64 logits of rows given as (first entry, length), entry by entry in stored order -- or,
    with ``rng``, entries and factors in a shuffled order."""
    k = V.shape[1]
    fperm = rng.permutation(k) if rng is not None else np.arange(k)
    z = np.full(len(begin), w0[0])
    for L in np.unique(length):
        if L == 0:
            continue
        rows = np.flatnonzero(length == L)
        order = rng.permutation(L) if rng is not None else np.arange(L)
        q, lin, s2 = np.zeros((len(rows), k)), np.zeros(len(rows)), np.zeros((len(rows), k))
        for j in order:
            c, xv = cols[begin[rows] + j], x[begin[rows] + j]
            vx = V[c][:, fperm] * xv[:, None]
            q += vx
            s2 += vx * vx
            lin += w[c] * xv
        pair = np.cumsum(q * q - s2, axis=1)[:, -1]  # (sequential over the factors)
        z[rows] = w0[0] + lin + 0.5 * pair
    return z


def _log_rows(log):
    X = log["features"]
    return X.indptr[:-1].astype(np.int64), np.diff(X.indptr).astype(np.int64), X.indices, X.data


def _terms64(pred, y, p, eps=fr.EPS):
    r = y / p
    return r * np.log(pred + eps) + (1 - r) * np.log(1 - pred + eps)


def _term_excess(pred, y, p, o, k, y_true, eps=fr.EPS):
    """Per row: |float64 loss term - oracle term| / (tau + u sum |term|): the row's own part of the
    loss tolerance and the whole allowance of the mean's sum (the oracle with the true labels)."""
    r = np.asarray(y_true).astype(LD) / np.asarray(p).astype(LD)
    a, b = r * np.log(o.p + LD(eps)), (1 - r) * np.log(1 - o.p + LD(eps))
    tp = fr.tol_p(o, k)
    tau = (np.abs(r) * tp / (o.p + LD(eps)) + np.abs(1 - r) * tp / (1 - o.p + LD(eps))
           + 4 * LD(fr.U) * (np.abs(a) + np.abs(b)))
    got = _terms64(pred, np.asarray(y, dtype=np.float64), p, eps)
    return (np.abs(got.astype(LD) - (a + b)) / (tau + LD(fr.U) * np.abs(a + b).sum())).astype(np.float64)


@pytest.mark.parametrize("k", [8, 13, 128, 300])
def test_oracle_equals_the_dense_long_double_logit_and_the_float64_reference(k):
    log, theta, o = fr.case(k, 400, (16,), ((40, 41),))
    X = log["features"]
    z_dense, _ = gf.fm_logit_ld(X.toarray().astype(LD), LD(theta[0][0]), theta[1].astype(LD), theta[2].astype(LD))
    eps_ld = float(np.finfo(LD).eps)
    assert (np.abs(o.z - z_dense) <= (2 * o.length + k + 16) * eps_ld * o.S_z).all()
    np.testing.assert_array_equal(o.length, np.diff(X.indptr))
    # float64 rounding: the reference's scores and loss inside half of the tolerances
    fr.assert_scores(cpu_ref.fm_predict(X, *theta), o, k, "cpu_ref.fm_predict", bound=0.5)
    z64 = cpu_ref.fm_logit(X, *theta)
    assert (np.abs(z64 - o.z) <= 0.5 * fr.tol_z(o, k)).all()
    want, tol = fr.loss_oracle(o, k, log["labels"], log["pscores"])
    got = cpu_ref.ips_logloss(log["labels"].astype(np.float64), cpu_ref.fm_predict(X, *theta), log["pscores"])
    fr.assert_loss(got, want, tol, "cpu_ref.ips_logloss", bound=0.5)


@pytest.mark.parametrize("k", KS, ids=[gf.class_id(k) for k in KS])
def test_every_input_is_unsaturated_and_a_shuffled_float64_pass_stays_below_half(k):
    rng = np.random.default_rng(k)
    for name, log, theta, o in _inputs(k):
        assert fr.unsaturated_share(o) >= 0.8, (name, fr.unsaturated_share(o))
        assert np.isfinite(o.p).all()
        if name == "rows":  # (the gradient cases' logs carry no such rows)
            assert (np.abs(o.z) > fr.CLIP).sum() >= 4 and ((np.abs(o.z) > 39) & (np.abs(o.z) < 41)).sum() >= 4
        assert o.length[0] == 0 and o.length[-1] == 0 and (o.length == 0).sum() > 10
        for order in (None, rng):
            z = _rows64(*_log_rows(log), *theta, rng=order)
            worst_z = float(np.max(np.abs(z - o.z) / fr.tol_z(o, k)))
            pred = cpu_ref.sigmoid(z)
            worst_p = float(np.max(fr.score_excess(pred, o, k)))
            want, tol = fr.loss_oracle(o, k, log["labels"], log["pscores"])
            got = cpu_ref.ips_logloss(log["labels"].astype(np.float64), pred, log["pscores"])
            worst_l = float(abs(LD(got) - want) / tol)
            assert worst_z < 0.5 and worst_p < 0.5 and worst_l < 0.5, (name, worst_z, worst_p, worst_l)


@pytest.mark.parametrize("k,lpr", TRAIN_CASES)
def test_training_and_validation_logs_are_unsaturated(k, lpr):
    # (the row counts of the device cases that do not depend on the device)
    for n_rows, max_len, seed in ((600, None, 11), (100, None, 12), (300, None, 11), (30, None, 12), (1500, None, 11),
                                  (600, lpr, 11), (100, lpr, 12)):
        log, theta, o = fr.case(k, n_rows, (), (), max_len, seed, lpr)
        assert fr.unsaturated_share(o) >= 0.8 and np.isfinite(o.p).all(), (n_rows, max_len, fr.unsaturated_share(o))
        z = _rows64(*_log_rows(log), *theta, rng=np.random.default_rng(k))
        assert float(np.max(fr.score_excess(cpu_ref.sigmoid(z), o, k))) < 0.5


def _pick(o, log, need):
    """First row t in the unsaturated middle for which need(t) holds."""
    ok = (o.p > 0.05) & (o.p < 0.95)
    for t in np.flatnonzero(ok[:-1]):
        if need(int(t)):
            return int(t)
    raise AssertionError("no row for the mutation")


@pytest.mark.parametrize("k", [8, 13, 64, 128, 300, 513])
def test_mutations_break_the_tolerance_on_the_affected_row_only(k):
    (name, log, theta, o), = [c for c in _inputs(k) if c[0] == "rows"]
    begin, length, cols, x = _log_rows(log)
    y, p = log["labels"].astype(np.float64), log["pscores"]
    lpr = gf.CLASS_OF[k][0]

    def scores(begin, length, cols, x):
        return cpu_ref.sigmoid(_rows64(begin, length, cols, x, *theta))

    def assert_only(pred, rows, what):
        ex = fr.score_excess(pred, o, k)
        bad = np.flatnonzero(~(ex <= 1.0))
        np.testing.assert_array_equal(bad, np.sort(rows), err_msg=what)

    assert_only(scores(begin, length, cols, x), [], "no mutation")
    # 1. one entry of one row dropped (its last: the row is one entry short)
    t = _pick(o, log, lambda t: length[t] >= lpr + 1)
    l1 = length.copy()
    l1[t] -= 1
    assert_only(scores(begin, l1, cols, x), [t], "an entry dropped")
    # 2. a row scored with its neighbour's length (it reads on into the next row, or stops short)
    t = _pick(o, log, lambda t: length[t] >= 1 and length[t + 1] >= 1 and length[t] != length[t + 1])
    l2 = length.copy()
    l2[t] = length[t + 1]
    assert_only(scores(begin, l2, cols, x), [t], "the neighbour's length")
    # 3. a row's padding entry (its own last entry again) added with its true x
    t = _pick(o, log, lambda t: length[t] in (lpr - 1, lpr + 1, 2 * lpr + 1))
    at = begin[t] + length[t]
    cols3, x3 = np.insert(cols, at, cols[at - 1]), np.insert(x, at, x[at - 1])
    b3, l3 = begin + (np.arange(len(begin)) > t), length.copy()
    l3[t] += 1
    assert_only(scores(b3, l3, cols3, x3), [t], "a padding entry with its x")
    # 4. two neighbouring rows' labels swapped: the scores hold, the two rows' loss terms do not
    t = _pick(o, log, lambda t: y[t] != y[t + 1] and 0.05 < o.p[t + 1] < 0.95)
    y4 = y.copy()
    y4[[t, t + 1]] = y4[[t + 1, t]]
    pred = scores(begin, length, cols, x)
    assert (_term_excess(pred, y, p, o, k, y) <= 1.0).all()
    bad = np.flatnonzero(~(_term_excess(pred, y4, p, o, k, y) <= 1.0))
    np.testing.assert_array_equal(bad, [t, t + 1], err_msg="labels swapped")
    # ... and, the rows' propensities differing, so does the mean loss
    want, tol = fr.loss_oracle(o, k, y, p)
    fr.assert_loss(cpu_ref.ips_logloss(y, pred, p), want, tol, "unmutated")
    assert p[t] != p[t + 1]
    assert abs(LD(cpu_ref.ips_logloss(y4, pred, p)) - want) > tol


def test_tolerance_helpers_reject_what_they_must():
    log, theta, o = fr.case(8, 400, (16,), ((40, 41),))
    good = o.p.astype(np.float64)
    fr.assert_scores(good, o, 8, "exact")
    for t, v in ((5, np.nan), (5, np.inf), (200, good[200] * (1 + 1e-9))):
        bad = good.copy()
        bad[t] = v
        with pytest.raises(AssertionError, match=f"worst row {t} "):
            fr.assert_scores(bad, o, 8, "mutated")
    # a non-finite oracle row wants a non-finite score
    V = theta[2].copy()
    c = log["features"].indices[0]
    V[c, 0] = np.nan
    on = fr.row_oracle(log["features"], theta[0], theta[1], V)
    holds = np.asarray((log["features"][:, c] != 0).todense()).ravel()
    np.testing.assert_array_equal(~np.isfinite(on.p), holds)
    with pytest.raises(AssertionError):
        fr.assert_scores(good, on, 8, "finite where NaN is due")
    mixed = np.where(holds, np.nan, good)
    fr.assert_scores(mixed, on, 8, "NaN where due")
