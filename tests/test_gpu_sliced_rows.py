"""The sliced FM forward (fm_logit_slices_kernel, rfm_fm_sliced.hpp) row by row against the
long-double oracle of forward_rows_common.py, on the logs of sliced_rows_common.py: rows of a chosen
number of cached and uncached entries, cached-column counts at their edges, launches at the edges of
a wavefront's trip, the training rows of rfm_fm_train, non-finite parameters.  Needs an MI355X:
``pytest -m gpu``.

Every test runs with RFM_SLICED_MIN_ROWS=1 and asserts the shape it means -- the plan's slices, cached
columns and their LDS order (rfm_fm_plan_sliced, rfm_fm_plan_sliced_columns), the launch's workgroups
and rows per workgroup (rfm_fm_sliced_geometry) -- before it compares anything; sizes come from those
queries, not from a CU count written here.  Scores come through rfm_fm_plan_forward and are held to
forward_rows_common's derived tol_p, losses to its loss_oracle.

A  the class logs at every slice shape of SLICE_TABLE; registered in slot 1 = translated per call.
B  0, 1, 127, 128, 129 cached columns, the LDS cap and past it.
C  prefixes of the class log, and -- tiled from an oracle-checked log of 1 021 rows -- the smallest
   launches in which a wavefront takes 65 and 129 rows (the re-entry of its pipeline).
D  log A of the launch: rfm_fm_train with lr = 0 at batches of 1, 2 and 17 rows.
E  NaN / Inf in V and w: exactly the rows that hold the column are non-finite."""
import numpy as np
import pytest
from scipy.sparse import csr_matrix

import forward_rows_common as fr
import grad_forms_common as gf
import sliced_rows_common as sr

pytestmark = pytest.mark.gpu

SECOND_PASS_MAX_ROWS = 150_000   # as test_gpu_forward_rows.py
CASES_A = [(64, k) for k in sr.SLICE_TABLE] + [(16, 130), (16, 300), (32, 130), (32, 300)]
CASES_B = [(F, 130) for F in (0, 1, 127, 128, 129, 151, 156)] + [(76, 256), (80, 256)]


@pytest.fixture(scope="module")
def rt():
    from relevance_factorizationmachine_amd import runtime
    return runtime.Runtime.get()


@pytest.fixture(autouse=True)
def _sliced_from_one_row(monkeypatch):
    monkeypatch.setenv("RFM_SLICED_MIN_ROWS", "1")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _assert_plan(plan, k, ML, cached):
    """The plan is the one the case is built for: slices, records per row, the cached columns in
    their LDS order."""
    ns, sw, _ = sr.slices_of(k)
    assert plan.sliced() == {"slices": ns, "factors_per_slice": sw, "cached_columns": len(cached),
                             "records_per_row": ML}, plan.sliced()
    np.testing.assert_array_equal(plan.sliced_columns(), cached)


def _geometry(plan, n, k, n_cached):
    """rfm_fm_sliced_geometry of a launch of n rows, checked for what the kernel relies on."""
    ns, sw, _ = sr.slices_of(k)
    g = plan.sliced_geometry(n)
    assert g["sliced"] == 1, g
    wps = g["workgroups"] // 8 * (8 // ns)        # workgroups of one slice
    assert g["workgroups"] % 8 == 0 and wps >= 1 and wps * g["rows_per_workgroup"] >= n, g
    assert g["lds_bytes"] == (n_cached + 1) * (8 * sw + 16) + 2048 <= 160 << 10, g
    g["per_slice"] = wps
    return g


def test_geometry_query_reads_the_switches_as_the_call_does(rt, monkeypatch):
    """rfm_fm_sliced_geometry: the default threshold of 4 096 rows, form_rows deciding for a shard,
    RFM_SLICED_LOSS=0, a plan without slices; and rfm_fm_plan_forward then scores the same rows in
    either form inside the tolerance."""
    ML, k = 16, 130
    log, nh, ng, theta, o = sr.class_case(ML, k)
    tlog, C, _ = sr.train_log(sr.N_FREQ, sr.N_RARE, ML)
    n = log["features"].shape[0]
    dev, plain = gf.DeviceLog(rt, tlog, k, 64), gf.DeviceLog(rt, tlog, 128, 64)
    try:
        assert plain.plan.sliced()["slices"] == 0 and plain.plan.sliced_geometry(n)["sliced"] == 0
        assert len(plain.plan.sliced_columns()) == 0
        at_one = dev.plan.sliced_geometry(n)
        assert at_one["sliced"] == 1
        ev, params = fr.DeviceRows(rt, log), gf.Params(rt, *theta)
        sliced = sr.plan_forward(rt, dev.plan, ev, params, n)
        monkeypatch.delenv("RFM_SLICED_MIN_ROWS")
        assert dev.plan.sliced_geometry(n)["sliced"] == 0 and dev.plan.sliced_geometry(4095)["sliced"] == 0
        assert dev.plan.sliced_geometry(4096)["sliced"] == 1
        assert dev.plan.sliced_geometry(n, 4096) == at_one   # (a shard of a log of 4 096 rows)
        assert dev.plan.sliced_geometry(4096, n)["sliced"] == 0
        unsliced = sr.plan_forward(rt, dev.plan, ev, params, n)   # (the plain forward)
        fr.assert_scores(unsliced, o, k, "below the threshold")
        fr.assert_scores(sliced, o, k, "sliced")
        monkeypatch.setenv("RFM_SLICED_MIN_ROWS", "1")
        monkeypatch.setenv("RFM_SLICED_LOSS", "0")
        assert dev.plan.sliced_geometry(n)["sliced"] == 0
    finally:
        dev.close()
        plain.close()


# --------------------------------------------------------------------------
# A. every slice shape
# --------------------------------------------------------------------------
@pytest.mark.parametrize("ML,k", CASES_A)
def test_class_log_row_by_row_at_every_slice_shape(rt, ML, k):
    """k = 130: pair 1 with one live lane; 256, 512, 1024: both pairs full; 258: a last slice whose
    pair 1 is wholly idle; 514: idle lanes inside pair 0; 1022: one idle lane in pair 1."""
    log, nh, ng, theta, o = sr.class_case(ML, k)
    tlog, C, _ = sr.train_log(sr.N_FREQ, sr.N_RARE, ML)
    n = log["features"].shape[0]
    dev = gf.DeviceLog(rt, tlog, k, 64)
    try:
        _assert_plan(dev.plan, k, ML, C.freq)
        g = _geometry(dev.plan, n, k, sr.N_FREQ)
        inside = sr.pairs_inside(sr.kind_masks(nh, ng, ML), g["rows_per_workgroup"])
        assert inside.all(), (g, [(sr.KINDS[a], sr.KINDS[b]) for a, b in zip(*np.nonzero(~inside))])
        ev, params = fr.DeviceRows(rt, log), gf.Params(rt, *theta)
        got = sr.plan_forward(rt, dev.plan, ev, params, n)
        fr.assert_scores(got, o, k, f"ML={ML} k={k}, translated per call")
        reg = sr.plan_forward(rt, dev.plan, ev, params, n, register=True)
        np.testing.assert_array_equal(_bits(reg), _bits(got), err_msg="registered in slot 1")
        again = sr.plan_forward(rt, dev.plan, ev, params, n)
        np.testing.assert_array_equal(_bits(again), _bits(got), err_msg="translated per call, again")
    finally:
        dev.close()


# --------------------------------------------------------------------------
# B. cached columns at their edges
# --------------------------------------------------------------------------
@pytest.mark.parametrize("F,k", CASES_B)
def test_cached_column_counts_at_their_edges(rt, F, k):
    ns, sw, _ = sr.slices_of(k)
    cap = sr.lds_cap(sw)
    H = min(F, cap)
    tlog, C, _ = sr.train_log(F, sr.EDGE_RARE, 64)
    log, marked = sr.edge_log(F, H)
    theta = sr.theta(k, C.n)
    o = fr.row_oracle(log["features"], *theta)
    n = log["features"].shape[0]
    dev = gf.DeviceLog(rt, tlog, k, 64)
    try:
        assert dev.plan.sliced()["cached_columns"] == H == min(F, cap)
        _assert_plan(dev.plan, k, 64, C.freq[:H])
        _geometry(dev.plan, n, k, H)
        if "cut" in marked:   # the first column past the cap is frequent and not cached
            assert marked["cut"] == C.freq[cap] and marked["cut"] not in dev.plan.sliced_columns()
        got = sr.plan_forward(rt, dev.plan, fr.DeviceRows(rt, log), gf.Params(rt, *theta), n)
        fr.assert_scores(got, o, k, f"F={F} k={k}")
    finally:
        dev.close()


# --------------------------------------------------------------------------
# C. trips
# --------------------------------------------------------------------------
def _find(plan, k, rows, want):
    for n in rows:
        g = plan.sliced_geometry(n)
        ns = sr.slices_of(k)[0]
        if g["sliced"] == 1 and want(n, g["rows_per_workgroup"], g["workgroups"] // 8 * (8 // ns)):
            return n
    raise AssertionError("no such launch")


def test_prefixes_of_the_class_log(rt):
    ML, k = 64, 300
    log, nh, ng, theta, o = sr.class_case(ML, k)
    tlog, C, _ = sr.train_log(sr.N_FREQ, sr.N_RARE, ML)
    N = log["features"].shape[0]
    dev = gf.DeviceLog(rt, tlog, k, 64)
    try:
        _assert_plan(dev.plan, k, ML, C.freq)
        ev, params = fr.DeviceRows(rt, log), gf.Params(rt, *theta)
        full = sr.plan_forward(rt, dev.plan, ev, params, N)
        fr.assert_scores(full, o, k, "the whole log")
        # whole workgroups without a row; a last workgroup of one row
        idle = _find(dev.plan, k, range(3, N), lambda n, rpw, wps: (wps - 1) * rpw >= n)
        single = _find(dev.plan, k, range(N - 1, 2, -1), lambda n, rpw, wps: n > rpw and n % rpw == 1)
        for n in (1, 2, 15, 16, 17, 127, 128, 129, idle, single):
            _geometry(dev.plan, n, k, sr.N_FREQ)
            got = sr.plan_forward(rt, dev.plan, ev, params, n)
            fr.assert_scores(got, o.take(slice(0, n)), k, f"{n} rows")
            np.testing.assert_array_equal(_bits(got), _bits(full[:n]), err_msg=f"{n} rows against the whole log")
    finally:
        dev.close()


def test_wavefronts_of_65_and_129_rows(rt):
    """k = 514 (four slices): the smallest launches whose workgroups hold 16 * 64 + 1 and
    2 * 16 * 64 + 1 rows -- wavefront 0 then re-enters its pipeline with a block of one row -- tiled
    from the 1 021-row log (1 021 is prime: a row's copies fall on every wavefront and every place of
    a block).  Every copy carries the bits its row has in the launch of 1 021 rows."""
    ML, k, base = 64, 514, 1021
    log, nh, ng, theta, o = sr.class_case(ML, k, base - sr.class_log(ML)[0]["features"].shape[0])
    tlog, C, _ = sr.train_log(sr.N_FREQ, sr.N_RARE, ML)
    X = log["features"]
    assert X.shape[0] == base
    dev = gf.DeviceLog(rt, tlog, k, 64)
    try:
        _assert_plan(dev.plan, k, ML, C.freq)
        params = gf.Params(rt, *theta)
        small = sr.plan_forward(rt, dev.plan, fr.DeviceRows(rt, log), params, base)
        fr.assert_scores(small, o, k, "1 021 rows")
        counts = []
        for per_wave in (65, 129):
            want = 16 * (per_wave - 1) + 1
            lo, hi = 1, 1 << 22
            assert dev.plan.sliced_geometry(hi)["rows_per_workgroup"] >= want
            while lo < hi:   # (rows per workgroup do not fall as the rows grow, once every CU has one)
                mid = (lo + hi) // 2
                if dev.plan.sliced_geometry(mid)["rows_per_workgroup"] >= want:
                    hi = mid
                else:
                    lo = mid + 1
            g = _geometry(dev.plan, lo, k, sr.N_FREQ)
            assert g["rows_per_workgroup"] == want and sr.waves_rows(want) == per_wave, (lo, g)
            assert dev.plan.sliced_geometry(lo - 1)["rows_per_workgroup"] == want - 1
            print(f"{per_wave} rows per wavefront: {lo} rows, {g}")
            if lo <= SECOND_PASS_MAX_ROWS:
                counts.append(lo)
        assert counts, "not even 65 rows per wavefront within the row limit"
        reps = -(-max(counts) // base)
        indptr = np.concatenate([[0], (X.indptr[1:][None, :] + X.nnz * np.arange(reps)[:, None]).reshape(-1)])
        tiled = {"features": csr_matrix((np.tile(X.data, reps), np.tile(X.indices, reps), indptr),
                                        shape=(reps * base, X.shape[1])),
                 "labels": np.tile(log["labels"], reps), "pscores": np.tile(log["pscores"], reps)}
        ev = fr.DeviceRows(rt, tiled)
        for n in counts:
            got = sr.plan_forward(rt, dev.plan, ev, params, n)
            np.testing.assert_array_equal(_bits(got), _bits(small[np.arange(n) % base]), err_msg=f"{n} rows")
    finally:
        dev.close()


# --------------------------------------------------------------------------
# D. log A: the training rows of rfm_fm_train
# --------------------------------------------------------------------------
def _ids_d(named, batch, n_rows, rng):
    """Iterations whose loss each A-side branch decides: a long row (read from indptr_a), an empty
    row, ordinary rows through row_ids -- alone at batch 1, at both ends of the batch otherwise."""
    l65, l130 = named["long"]
    e0, e1, e2 = named["empty"]
    special = {l65, l130, e0, e1, e2, named["longest"]}
    plain = rng.permutation([r for r in range(n_rows) if r not in special])
    if batch == 1:
        return np.array([[l65], [l130], [e0], [plain[0]], [named["longest"]]], dtype=np.int32)
    its = []
    for first, last in ((l65, plain[0]), (plain[1], l130), (e0, l65), (l130, e1), (plain[2], e2), (plain[3], plain[4])):
        mid = plain[10: 10 + batch - 2] if batch > 2 else []
        its.append([first, *mid, last])
    if batch > 4:   # all of them in one batch, the long rows and an empty row in the middle
        body = [l65, e0, l130, e1, named["longest"], e2]
        fill = list(plain[40: 40 + batch - len(body)])
        its.append(fill[: len(fill) // 2] + body + fill[len(fill) // 2:])
    return np.array(its, dtype=np.int32)


CASES_D = [(300, 1, 1), (300, 2, 1), (300, 17, 16), (514, 1, 1), (514, 2, 1), (514, 17, 16), (514, 8, 26)]


@pytest.mark.parametrize("k,batch,n_val", CASES_D)
def test_training_rows_of_the_launch(rt, k, batch, n_val):
    """(514, 8, 26) is the launch in which a wavefront's block of ids holds rows of both logs: two
    workgroups of 17 rows per slice, wavefront 0 takes rows 0 (log A) and 16 (log B).  At (17, 16)
    the boundary between the logs falls where the queried geometry puts it -- with at most 17 rows to
    a workgroup, between two wavefronts' rows or between two workgroups."""
    tlog, C, named = sr.train_log(sr.N_FREQ, sr.N_RARE, 64, (65, 130), 3)
    clog = sr.class_log(64)[0]
    vlog = {"features": clog["features"][1: 1 + n_val], "labels": clog["labels"][1: 1 + n_val],
            "pscores": clog["pscores"][1: 1 + n_val]}
    theta = sr.theta(k, C.n)
    to, vo = fr.row_oracle(tlog["features"], *theta), fr.row_oracle(vlog["features"], *theta)
    assert [int(to.length[r]) for r in named["long"]] == [65, 130] and (to.length[named["empty"]] == 0).all()
    ids = _ids_d(named, batch, tlog["features"].shape[0], np.random.default_rng(k + batch))
    assert ids.shape[1] == batch and all(len(set(b)) == batch for b in ids.tolist())
    dev = gf.DeviceLog(rt, tlog, k, 64)
    try:
        _assert_plan(dev.plan, k, 64, C.freq)
        g = _geometry(dev.plan, batch + n_val, k, sr.N_FREQ)
        if (batch, n_val) == (8, 26):
            rpw = g["rows_per_workgroup"]
            assert any(t // rpw == (t + 16) // rpw and t + 16 < batch + n_val for t in range(batch - 16, batch) if t >= 0), g
        val = fr.DeviceRows(rt, vlog)
        forms = fr.train_forms(rt, dev.plan, batch, len(ids), 0, val, n_val)
        assert forms["sliced"] == 1 and forms["merged"] == 0, forms
        tl, vl = fr.train_lr0(rt, dev, gf.Params(rt, *theta), ids, val)
        want_v, tol_v = fr.loss_oracle(vo, k, vlog["labels"], vlog["pscores"])
        for it, b in enumerate(ids):
            want, tol = fr.loss_oracle(to.take(b), k, tlog["labels"][b], tlog["pscores"][b])
            fr.assert_loss(tl[it], want, tol, f"train loss of iteration {it} (rows {b.tolist()})")
            fr.assert_loss(vl[it], want_v, tol_v, f"validation loss of iteration {it}")
    finally:
        dev.close()


# --------------------------------------------------------------------------
# E. non-finite values
# --------------------------------------------------------------------------
def test_non_finite_values_reach_exactly_the_rows_that_hold_the_column(rt):
    """k = 300: slices of 150 factors, so pair 1 of a cached row's LDS read runs 848 bytes into the
    NEXT cached column's row -- a non-finite value there must not reach a row that holds only the
    column before it.  Column 0 is what empty rows, long rows and absent gathers read and drop."""
    ML, k = 64, 300
    log, nh, ng, theta, o = sr.class_case(ML, k)
    tlog, C, _ = sr.train_log(sr.N_FREQ, sr.N_RARE, ML)
    X = log["features"]
    n = X.shape[0]
    row_of = np.repeat(np.arange(n), np.diff(X.indptr))
    rank = np.full(C.n, -1)
    rank[C.freq] = np.arange(sr.N_FREQ)
    # a row that holds one cached column alone, and the column stored next after it
    alone = [int(r) for r in np.flatnonzero((nh == 1) & (ng == 0)) if rank[X.indices[X.indptr[r]]] < sr.N_FREQ - 1]
    assert alone
    after = int(C.freq[rank[X.indices[X.indptr[alone[0]]]] + 1])
    rare_counts = np.bincount(X.indices, minlength=C.n)[C.rare]
    places = {"column 0": 0, "the first cached column": int(C.freq[0]), "the column stored after a lone one": after,
              "a rare column": int(C.rare[np.argmax(rare_counts)])}
    assert rank[0] < 0 and o.length[0] == 0 and (o.length > ML).any()
    dev = gf.DeviceLog(rt, tlog, k, 64)
    try:
        _assert_plan(dev.plan, k, ML, C.freq)
        _geometry(dev.plan, n, k, sr.N_FREQ)
        ev = fr.DeviceRows(rt, log)
        for name, col in places.items():
            holds = np.zeros(n, dtype=bool)
            holds[row_of[X.indices == col]] = True
            assert 0 < holds.sum() < n // 2 and not holds[alone[0]] and not holds[o.length == 0].any(), name
            z = o.z.copy()
            z[holds] = np.nan
            want = fr.Rows(z, o.S_z, o.length)
            for value in (np.nan, np.inf):
                w0, w, V = theta[0], theta[1].copy(), theta[2].copy()
                w[col], V[col, :] = value, value
                got = sr.plan_forward(rt, dev.plan, ev, gf.Params(rt, w0, w, V), n)
                np.testing.assert_array_equal(~np.isfinite(got), holds, err_msg=f"{name} = {value}")
                fr.assert_scores(got, want, k, f"{name} = {value}")
    finally:
        dev.close()
