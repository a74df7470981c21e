"""Shared by the tests of the device grouping of fold-in examples (test_fold_group_host.py,
test_gpu_fold_group.py): a NumPy statement of the device scheme -- count, scan, place at
a cursor in a chosen ARRIVAL ORDER, order each bin (sort up to the cap, walk all keys beyond it) -- with
the four mistakes the kernels can make, a restatement of the launch shapes and the workspace, the case
list, and wrappers of the raw ABI call that keep every output between sentinels.  Importing this module
touches neither the GPU nor the library under test.

The comparison target everywhere is ``fold.fold_examples`` on the same data: ``row_ptr``, ``ids``,
``ry`` and ``order`` equal in dtype and value, ``ry`` in bits.  There is no tolerance: the grouping moves
integers, and ``ry`` is one IEEE double division per example on either side."""
import functools
import types
import zlib

import numpy as np

import fold_common
import mf_step_common as ms

CAP = 2048            # rfm_fold_group.hip kCap: the longest bin ordered in LDS
WAVE_CAP = 256        # kWaveCap: the longest bin a wavefront orders
BLOCK = 256           # kFgBlock
LONG_BLOCK = 1024     # kLongBlock
WAVES = BLOCK // 64
PER_CU = 8            # kPerCu
SCAN_TILE = BLOCK * 8
N_FIXED = fold_common.N_FIXED
SENTINEL = 0x5A       # every byte of an output buffer before the call


# --------------------------------------------------------------------------
# the device scheme, stated in NumPy
# --------------------------------------------------------------------------
ARRIVALS = {
    "identity": lambda n, rng: np.arange(n),
    "reversed": lambda n, rng: np.arange(n)[::-1],
    "random": lambda n, rng: rng.permutation(n),
}


def group_np(keys, n_bins, arrival, cap=CAP, mutation=None):
    """``(bin_ptr int64 [n_bins + 1], perm int32)`` of keys in [0, n_bins) (-1: left out) as the device
    makes them; ``arrival``: the order in which the placements reach their cursors.  Mutations:
    "arrival_order" = the bins are left as placed; "ties_high" = a bin is ordered descending."""
    keys = np.asarray(keys, dtype=np.int64)
    kept = keys >= 0
    counts = np.bincount(keys[kept], minlength=n_bins)
    bin_ptr = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    perm = np.full(int(bin_ptr[-1]), -1, dtype=np.int32)
    cursor = np.zeros(n_bins, dtype=np.int64)
    for i in arrival:
        b = keys[i]
        if b >= 0:
            perm[bin_ptr[b] + cursor[b]] = i
            cursor[b] += 1
    if mutation == "arrival_order":
        return bin_ptr, perm
    for b in np.flatnonzero(counts >= 2):
        lo, hi = bin_ptr[b], bin_ptr[b + 1]
        if hi - lo <= cap:
            perm[lo:hi] = np.sort(perm[lo:hi])
        else:  # the walk: every key in input order, the matches compacted
            perm[lo:hi] = np.flatnonzero(keys == b)
        if mutation == "ties_high":
            perm[lo:hi] = perm[lo:hi][::-1]
    return bin_ptr, perm


def fold_group_np(data, n_new, n_fixed, new_col, arrival="identity", cap=CAP, mutation=None, seed=0):
    """rfm_fold_group in NumPy: ``((row_ptr, ids, ry, order), status)``.  Mutations: those of
    ``group_np`` ("arrival_order" in the examples' pass, "ties_high" in the rows' pass),
    "order_ascending" = rows by ascending count, "ry_by_position" = ``ry`` not gathered by ``perm``."""
    rng = np.random.default_rng(seed)
    pairs = np.asarray(data["features"])
    n = pairs.shape[0]
    new, other = pairs[:, new_col].astype(np.int64), pairs[:, 1 - new_col].astype(np.int64)
    bad_new, bad_other = (new < 0) | (new >= n_new), (other < 0) | (other >= n_fixed)
    bad = bad_new | bad_other
    status = np.array([bad_new.sum(), bad_other.sum(), np.flatnonzero(bad)[0] if bad.any() else -1, 0], dtype=np.int32)
    keys = np.where(bad, -1, new)
    row_ptr, perm = group_np(keys, n_new, ARRIVALS[arrival](n, rng), cap,
                             mutation if mutation == "arrival_order" else None)
    q = np.asarray(data["labels"]).astype(np.float64) / np.asarray(data["pscores"]).astype(np.float64)
    ry = q[: len(perm)] if mutation == "ry_by_position" else q[perm]
    counts = np.diff(row_ptr)
    keys2 = counts if mutation == "order_ascending" else n - counts
    _, order = group_np(keys2, n + 1, ARRIVALS[arrival](n_new, rng), cap, mutation if mutation == "ties_high" else None)
    return (row_ptr, other[perm].astype(np.int32), ry, order), status


def filtered(data, n_new, n_fixed, new_col):
    """``data`` without the examples whose ids are out of range: what the device groups."""
    pairs = np.asarray(data["features"])
    new, other = pairs[:, new_col], pairs[:, 1 - new_col]
    keep = (new >= 0) & (new < n_new) & (other >= 0) & (other < n_fixed)
    return {k: np.asarray(v)[keep] for k, v in data.items()}


def assert_same(got, want, what):
    """The four arrays of ``fold_examples``, equal in dtype and value, ``ry`` in bits."""
    for name, g, w in zip(("row_ptr", "ids", "ry", "order"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if name == "ry":
            g, w = g.view(np.uint64), w.view(np.uint64)
        np.testing.assert_array_equal(g, w, err_msg=f"{what}: {name}")


def differs(got, want):
    """The names of the arrays that differ."""
    out = []
    for name, g, w in zip(("row_ptr", "ids", "ry", "order"), got, want):
        if g.shape != w.shape or not np.array_equal(np.asarray(g).view(np.uint64 if name == "ry" else g.dtype),
                                                    np.asarray(w).view(np.uint64 if name == "ry" else w.dtype)):
            out.append(name)
    return out


# --------------------------------------------------------------------------
# launch shapes and workspace, restated (rfm_fold_group.hip grids_for, Workspace)
# --------------------------------------------------------------------------
def _capped(items, per_wg, n_cu, floor):
    return max(floor, min(-(-items // per_wg), n_cu * PER_CU))


def geometry_py(n, n_bins, n_cu=ms.ASSUMED_CUS):
    return dict(cap=CAP, block=BLOCK, bin_grid=_capped(n_bins, WAVES, n_cu, 1), wave_cap=WAVE_CAP,
                mid_grid=_capped(n // (WAVE_CAP + 1), 1, n_cu, 0), long_grid=_capped(n // (CAP + 1), 1, n_cu, 0),
                long_block=LONG_BLOCK, key_grid=_capped(n, BLOCK, n_cu, 1))


def workspace_py(n, n_new):
    al = lambda b: (b + 15) // 16 * 16
    hist_words = max(n_new, n + 1) + 1
    list_cap = max(n, n_new) // (WAVE_CAP + 1) + 1
    parts = [n * 4, n * 4, hist_words * 4, n_new * 4, (n + 2) * 8, (-(-hist_words // SCAN_TILE) + 1) * 8,
             (4 + 2 * list_cap) * 4]
    return max(16, sum(al(b) for b in parts))


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------
def _case(name, new, n_new, n_fixed=N_FIXED, new_col=0, labels=None, pscores=None, other=None):
    rng = np.random.default_rng(zlib.crc32(name.encode()))
    new = np.asarray(new, dtype=np.int64)
    n = len(new)
    other = rng.integers(0, max(n_fixed, 1), size=n) if other is None else np.asarray(other, dtype=np.int64)
    labels = (rng.random(n) < 0.5).astype(np.float64) if labels is None else labels
    pscores = rng.uniform(0.1, 1.0, size=n) ** 0.5 if pscores is None else pscores
    cols = (new, other) if new_col == 0 else (other, new)
    feats = np.stack(cols, axis=1) if n else np.zeros((0, 2), dtype=np.int64)
    return types.SimpleNamespace(name=name, n=n, n_new=n_new, n_fixed=n_fixed, new_col=new_col,
                                 data={"features": feats, "labels": labels, "pscores": pscores})


def _shuffled(name, lengths):
    rng = np.random.default_rng(zlib.crc32(("shuffle-" + name).encode()))
    return rng.permutation(np.repeat(np.arange(len(lengths)), lengths))


def lognormal_lengths(n_rows=700):
    """About 50 000 examples; every tier of the per-bin ordering is live: rows of 0, 1, 2..WAVE_CAP,
    WAVE_CAP+1..CAP and one beyond the cap."""
    rng = np.random.default_rng(19)
    lengths = np.minimum(rng.lognormal(3.4, 1.3, size=n_rows).astype(np.int64), CAP)
    lengths[:6] = [0, 1, WAVE_CAP, WAVE_CAP + 1, CAP, CAP + 905]
    return rng.permutation(lengths)


def many_bins(n_cu=ms.ASSUMED_CUS):
    """37 more non-empty rows than one turn of the per-bin grid takes, two examples each."""
    return n_cu * PER_CU * WAVES + 37


@functools.lru_cache(maxsize=None)
def group_cases(n_cu=ms.ASSUMED_CUS):
    out = [
        _case("n0", [], 5),
        _case("n0-nnew0", [], 0),
        _case("n1", [2], 4),
        *(_case(f"one-row-{n}", np.full(n, 1), 3) for n in (CAP - 1, CAP, CAP + 1)),
        _case("reversed-singles", np.arange(CAP + 1)[::-1], CAP + 1),          # the long bin in the order pass
        _case("empty-rows", _shuffled("empty-rows", [0, 3, 2, 0, 0, 5, 1, 0]), 8),  # first, middle, last
        _case("equal-counts", _shuffled("equal-counts", [5] * 37), 37),
        _case("lognormal", _shuffled("lognormal", lognormal_lengths()), 700),
        _case("many-bins", _shuffled("many-bins", [2] * many_bins(n_cu)), many_bins(n_cu)),
        _case("mixed", _shuffled("mixed", [(7 * r) % 90 for r in range(40)]), 40),
        _case("mixed-items", _shuffled("mixed", [(7 * r) % 90 for r in range(40)]), 40, new_col=1),
    ]
    rng = np.random.default_rng(3)
    n = 2000
    out.append(_case("inexact", rng.integers(0, 30, size=n), 30, labels=rng.normal(size=n),
                     pscores=rng.uniform(0.01, 1.0, size=n)))
    il = fold_common.FoldCaseBase("lognormal-interleaved", 8, fold_common._chains("lognormal-interleaved", lognormal_lengths()), 1)
    out.append(types.SimpleNamespace(name=il.name, n=int(il.lengths.sum()), n_new=il.n_new, n_fixed=il.n_fixed, new_col=0,
                                     data=il.data(interleaved=True)))
    return {c.name: c for c in out}


def bad_id_cases():
    """Ids out of range on either column, at the first and the last example (and one in between)."""
    out = {}
    base = group_cases()["mixed"]
    for col, which in ((0, "new"), (1, "other")):
        for new_col in (0, 1):
            feats = base.data["features"].copy() if new_col == 0 else base.data["features"][:, ::-1].copy()
            c = col if new_col == 0 else 1 - col
            limit = base.n_new if which == "new" else base.n_fixed
            feats[0, c], feats[-1, c], feats[base.n // 2, c] = -1, limit, limit + 7
            name = f"bad-{which}-col{new_col}"
            out[name] = types.SimpleNamespace(name=name, n=base.n, n_new=base.n_new, n_fixed=base.n_fixed, new_col=new_col,
                                              data={**base.data, "features": feats}, which=which)
    both = base.data["features"].copy()
    both[3] = [-5, base.n_fixed]                      # one example counted in both words
    both[9, 1] = -2
    out["bad-both"] = types.SimpleNamespace(name="bad-both", n=base.n, n_new=base.n_new, n_fixed=base.n_fixed, new_col=0,
                                            data={**base.data, "features": both}, which="new")
    return out


def want_of(case):
    from relevance_factorizationmachine_amd import fold
    return fold.fold_examples(case.data, case.n_new, case.n_fixed, case.new_col, 1)


# --------------------------------------------------------------------------
# the raw ABI call, every output between sentinels
# --------------------------------------------------------------------------
PAD = 8


class Fenced:
    """``n`` elements of ``dtype`` on the device, every byte a sentinel, with ``PAD`` more before and
    after; ``host()`` asserts those kept their bytes and returns the interior."""

    def __init__(self, rt, n, dtype):
        import torch
        self.n, self.dtype = n, np.dtype(dtype)
        self.dev = torch.full(((n + 2 * PAD) * self.dtype.itemsize,), SENTINEL, dtype=torch.uint8, device=rt.torch_device)

    @property
    def ptr(self):
        return self.dev.data_ptr() + PAD * self.dtype.itemsize

    def host(self):
        flat = self.dev.cpu().numpy()
        edge = PAD * self.dtype.itemsize
        assert (flat[:edge] == SENTINEL).all() and (flat[len(flat) - edge:] == SENTINEL).all(), "a sentinel changed"
        return flat[edge: len(flat) - edge].view(self.dtype).copy()


def run_group(rt, case, id_dtype=np.int64, layout="rows", workspace_extra=0):
    """rfm_fold_group on a case, twice: ``((row_ptr, ids, ry, order), status, kept)``, ``ids`` and ``ry``
    cut to the ``kept`` examples (what lies behind them must still be sentinels).  ``layout``: "rows" =
    an (N, 2) array, element stride 2; "columns" = two separate columns, stride 1.  Inputs must keep
    their bits, sentinels theirs, and the second call must give what the first gave."""
    import torch
    from relevance_factorizationmachine_amd import _lib, fold
    feats = np.ascontiguousarray(case.data["features"].astype(id_dtype))
    labels = np.ascontiguousarray(case.data["labels"], dtype=np.float64)
    pscores = np.ascontiguousarray(case.data["pscores"], dtype=np.float64)
    n, n_new, width = case.n, case.n_new, np.dtype(id_dtype).itemsize
    sent = np.ascontiguousarray(feats.T) if layout == "columns" else feats
    d_feats = rt.upload(sent if sent.size else np.zeros(2, id_dtype))
    d_labels, d_pscores = (rt.upload(a if a.size else np.zeros(1)) for a in (labels, pscores))
    stride, second = (1, n * width) if layout == "columns" else (2, width)
    cols = [d_feats.data_ptr() + c * second for c in (case.new_col, 1 - case.new_col)]
    n_bytes = fold.group_workspace(n, n_new)
    assert n_bytes == workspace_py(n, n_new)
    ws = torch.full((n_bytes + workspace_extra,), SENTINEL, dtype=torch.uint8, device=rt.torch_device)

    def once():
        out = [Fenced(rt, n_new + 1, np.int64), Fenced(rt, n, np.int32), Fenced(rt, n, np.float64),
               Fenced(rt, n_new, np.int32), Fenced(rt, 4, np.int32)]
        _lib.check(rt.lib.rfm_fold_group(rt.ctx, cols[0], cols[1], stride, width, d_labels.data_ptr(), d_pscores.data_ptr(),
                                         n, n_new, case.n_fixed, ws.data_ptr(), n_bytes, *(o.ptr for o in out)))
        rt.sync()
        return [o.host() for o in out]

    first, again = once(), once()
    for name, a, b in zip(("row_ptr", "ids", "ry", "order", "status"), first, again):
        np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=f"{case.name}: two calls differ in {name}")
    if workspace_extra:
        assert (ws.cpu().numpy()[n_bytes:] == SENTINEL).all(), "written past the workspace"
    for dev, host, what in ((d_feats, sent, "features"), (d_labels, labels, "labels"), (d_pscores, pscores, "pscores")):
        np.testing.assert_array_equal(dev.cpu().numpy().ravel()[: host.size].view(np.uint8), host.ravel().view(np.uint8),
                                      err_msg=f"{case.name}: {what} changed")
    row_ptr, ids, ry, order, status = first
    kept = int(row_ptr[-1])
    assert 0 <= kept <= n
    assert (ids[kept:].view(np.uint8) == SENTINEL).all() and (ry[kept:].view(np.uint8) == SENTINEL).all(), \
        "written behind the kept examples"
    return (row_ptr, ids[:kept], ry[:kept], order), status, kept


# --------------------------------------------------------------------------
# end to end: models around cases of fold_in_common.py and fm_fold_common.py
# --------------------------------------------------------------------------
def mf_model(case, side):
    """A model whose fixed side is the case's: folding the case in on ``side`` ("user": the items are
    fixed) runs the kernel on the case's chains."""
    import relevance_factorizationmachine_amd as pkg
    F, fb = case.fixed()
    other = (np.zeros((3, case.k)), np.zeros(3))
    (P, bu), (Q, bi) = ((other, (F, fb)) if side == "user" else ((F, fb), other))
    m = pkg.LogisticMatrixFactorization(estimator="IPS", n_epochs=1, n_factors=case.k, lr=ms.LR, batch_size=40, seed=3,
                                        n_users=P.shape[0], n_items=Q.shape[0], reg=ms.REG)
    for h, v in ((m.P, P), (m.Q, Q), (m.b_u, bu), (m.b_i, bi)):
        h.set(v)
    m.b = ms.B0
    return m


def fm_problem(case, side):
    """A catalogue [one-hot user | user table | one-hot item | item table] whose fixed side has the
    case's ``n_fixed`` rows, a model of random parameters on it and feature rows for the case's new
    rows: ``(model, sides, new_rows)``."""
    import relevance_factorizationmachine_amd as pkg
    import scipy.sparse as sp
    from relevance_factorizationmachine_amd import recommend as rec
    rng = np.random.default_rng(zlib.crc32(("fm-" + case.name + side).encode()))
    nu, ni = (4, case.n_fixed) if side == "user" else (case.n_fixed, 4)
    uw, iw = 4, 3

    def table(n, width):
        T = (rng.random((n, width)) < 0.6).astype(np.float64)
        T[:, 0] = 1.0
        return sp.csr_matrix(T)

    n_features = nu + uw + ni + iw
    XU = sp.hstack([sp.identity(nu), table(nu, uw), sp.csr_matrix((nu, ni + iw))]).tocsr()
    XI = sp.hstack([sp.csr_matrix((ni, nu + uw)), sp.identity(ni), table(ni, iw)]).tocsr()
    if side == "user":
        new_rows = sp.hstack([sp.csr_matrix((case.n_new, nu)), table(case.n_new, uw), sp.csr_matrix((case.n_new, ni + iw))])
    else:
        new_rows = sp.hstack([sp.csr_matrix((case.n_new, nu + uw + ni)), table(case.n_new, iw)])
    model = pkg.FactorizationMachines(estimator="IPS", n_epochs=1, n_factors=case.k, seed=5, n_features=n_features,
                                      lr=0.01, batch_size=40, alpha=0.3)
    model.w0.set(np.array([0.2]))
    model.w.set(rng.normal(scale=0.1, size=n_features))
    model.V.set(rng.uniform(-1.0, 1.0, size=(n_features, case.k)) * np.sqrt(1.0 / case.k))
    return model, rec.Sides(XU, XI), new_rows.tocsr()


def on_device(rt, data):
    """``data`` with every piece a tensor on the runtime's device."""
    return {k: rt.upload(np.ascontiguousarray(v)) for k, v in data.items()}
