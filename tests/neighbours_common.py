"""Shared by the neighbour tests (test_neighbours_host.py, test_gpu_neighbours.py;
rfm_rows_normalise and rfm_pair_topk_raw of csrc/rfm_pairs.hip, recommend.neighbours, DESIGN.md 8
N22): the long-double oracle of norms, normalised rows and cosines / dot products, a NumPy float64
statement of the normalisation kernel's exact order that carries four mutations, a host statement
of the lists that carries two more, the derived tolerances, the case lists, and the checker that
both the GPU tests and the mutation tests go through.  It reuses pair_tile_common (Pairs,
pair_oracle, oracle_lists, separated_share, assert_within, the sentinels).  Importing this module
touches neither the GPU nor the package under test.

With u = 2^-53, c = ceil(k / 64) and a row x of k factors whose squares neither overflow nor
underflow:

s       the kernel's sum of squares.  Every term is a rounded product (1 u) and goes through at
        most c adds of its lane (the first, to +0.0, is exact) and the 6 adds of the xor tree;
        all terms are >= 0, so s = S (1 + e), |e| <= (c + 7) u, S = sum_f x_f^2.
norm    sqrt halves the relative error and rounds once: |d norm| <= ((c + 7) / 2 + 1) u norm.
x^_f    one more rounding for the quotient: |d x^_f| <= E |x^_f|, E = ((c + 7) / 2 + 2) u
        (times 1 + 2^-40 for the second-order terms).  E is 6 u up to 64 factors, 9 u at 400.
cosine  the tile multiplies the COMPUTED rows, and is off by pair_oracle's tol_z = (kpad + 8) u
        S_z of them, S_z = sum_f |x^_f y^_f| (c = LU = LI = 0); the computed rows are off by E
        each, which moves the sum by at most (2 E + E^2) S_z.  tol = tol_z + 2 E (1 + 2^-40) S_z.
dot     the rows as they are: tol_z alone.

All derived, none measured.  The floor (test_neighbours_host.py): the float64 statement of the
kernel, on the factors as stored and on shuffled factors, and the float64 statement of the
tile's sum in both orders, stay below half of each tolerance on every case list the GPU tests
use.  (A sequential float64 sum over k factors is NOT bounded by E -- its bound grows with k, the
kernel's with log: the floor is taken with the kernel's own tree.)

Inputs: rows ~ N(0, 1).  At k = 1 every cosine is exactly +-1, so k = 1 is an exact-tie case and
no order case; the order cases are k >= 2, where the host test asserts that at least 99 % of the
adjacent positions of every query's oracle order are separated (pair_tile_common)."""
import functools

import numpy as np

import pair_tile_common as pc
from pair_tile_common import LD, U, pad4

LANES = 64
SECOND_ORDER = 1.0 + 2.0 ** -40
NORMALISE_MUTATIONS = ("squared_norm", "l1_norm", "drops_last_factor", "zero_rows_are_zero")
LIST_MUTATIONS = ("self_not_excluded", "sigmoid_values")

# rfm_rows_normalise, bit for bit
NORMALISE_FACTORS = (1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 400)
NORMALISE_ROWS = (1, 3, 4, 5, 257)
SPECIAL_ROWS = ("all zero", "a single non-zero", "-0.0", "a NaN", "an Inf", "1e200", "1e-200")
# neighbours through the raw ABI
NEIGHBOUR_ROWS = (129, 193)
NEIGHBOUR_FACTORS = (2, 5, 37, 400)
NEIGHBOUR_K = (1, 9, 64)
METRICS = ("cosine", "dot")
# rfm_pair_topk_raw at pair_tile_common.TILE_SHAPE
RAW_FACTORS = (5, 37)
HOST_FACTORS = (2, 3, 5, 37, 64, 400)  # of the separated-share test: the issue's list


def element_bound(k):
    """E: the relative error bound of a normalised element (module docstring)."""
    return ((-(-int(k) // LANES) + 7) / 2 + 2) * U * SECOND_ORDER


@functools.lru_cache(maxsize=None)
def rows(n, k, seed=0):
    """``[n, k]`` rows ~ N(0, 1): computed once, shared, read-only."""
    R = np.random.default_rng([n, k, seed, 77]).standard_normal((n, k))
    R.setflags(write=False)
    return R


def selection(n):
    """Query ids with repeats, in no order (the first and the last row among them)."""
    sel = np.array([n - 1, 0, 7, n // 2, 7, 64, 63, 0, n - 1, 65])
    return sel[sel < n]


def special_rows(k):
    """``[len(SPECIAL_ROWS), k]``: one row per name of SPECIAL_ROWS (the odd element last where k allows)."""
    R = np.random.default_rng(k).standard_normal((len(SPECIAL_ROWS), k))
    R[0] = 0.0
    R[1] = 0.0
    R[1, k - 1] = -1.75
    R[2, 0] = -0.0
    R[3, k // 2] = np.nan
    R[4, k - 1] = np.inf
    R[5] *= 1e200
    R[6] *= 1e-200
    return R


# --------------------------------------------------------------------------
# the long-double oracle
# --------------------------------------------------------------------------
def norms_ld(R):
    """``(norm [n], normalised rows [n, k])`` in np.longdouble; a row whose norm is zero or not finite,
    in long double or as float64 squares would have it, is NaN throughout."""
    R = np.asarray(R, dtype=np.float64)
    x = R.astype(LD)
    with np.errstate(all="ignore"):
        norm = np.sqrt((x * x).sum(axis=1))
        s64 = (R * R).sum(axis=1)  # (float64 squares: they overflow at 1e200 and vanish at 1e-200)
        ok = (norm > 0) & np.isfinite(norm) & (s64 > 0) & np.isfinite(s64)
        unit = np.where(ok[:, None], x / np.where(ok, norm, 1)[:, None], LD(np.nan))
    return norm, unit


def oracle(R, metric, queries=None):
    """``Pairs`` of every (query row, row of R): z = the cosine or the dot product in long double,
    S_z its magnitude, tol_z the derived tolerance of the module docstring.  ``queries`` None: R's own rows."""
    R = np.asarray(R, dtype=np.float64)
    Q = R if queries is None else np.asarray(queries, dtype=np.float64)
    k = R.shape[1]
    if metric == "cosine":
        a, b = norms_ld(Q)[1], norms_ld(R)[1]
    else:
        a, b = Q.astype(LD), R.astype(LD)
    with np.errstate(all="ignore"):
        z, S = a @ b.T, np.abs(a) @ np.abs(b).T
    bad = np.isnan(a).any(axis=1)[:, None] | np.isnan(b).any(axis=1)[None, :]
    z[bad], S[bad] = np.nan, np.nan
    o = pc.Pairs(z, S, pad4(k))
    if metric == "cosine":
        o.tol_z = o.tol_z + 2 * LD(element_bound(k)) * S
    return o


def self_mask(n):
    return np.eye(n, dtype=bool)


# --------------------------------------------------------------------------
# the float64 statement of the kernel
# --------------------------------------------------------------------------
def normalise_statement(M, k, mutation=None):
    """``(out [n, kpad], norm [n])`` of rfm_rows_normalise in float64, operation by operation as
    include/rfm_neighbours.h orders them: lane l starts from +0.0 and adds the rounded squares of the
    factors l, l + 64, ... in ascending order; the 64 sums go through the xor tree m = 32 .. 1; the
    root; one division per element; NaN for a norm that is zero, NaN or infinite; the padding zero.
    ``M`` is ``[n, >= k]`` (the row stride plays no part in the arithmetic).  ``mutation``:

    - squared_norm: the division is by s, not by its root;
    - l1_norm: the lanes add |x| for x^2;
    - drops_last_factor: when k % 64 == 1 the sum leaves out the last factor (the one chunk that
      only lane 0 enters);
    - zero_rows_are_zero: a row without a direction gives zeros, not NaN."""
    assert mutation is None or mutation in NORMALISE_MUTATIONS
    M = np.asarray(M, dtype=np.float64)[:, :k]
    n, chunks = M.shape[0], -(-k // LANES)
    with np.errstate(all="ignore"):
        X = np.zeros((n, chunks * LANES))  # (a lane without a factor adds +0.0, which changes no bit of a sum >= +0.0)
        X[:, :k] = M
        if mutation == "drops_last_factor" and k % LANES == 1:
            X[:, k - 1] = 0.0
        terms = np.abs(X) if mutation == "l1_norm" else X * X
        t = np.zeros((n, LANES))
        for j in range(chunks):
            t = t + terms[:, LANES * j: LANES * (j + 1)]
        lane = np.arange(LANES)
        for m in (32, 16, 8, 4, 2, 1):
            t = t + t[:, lane ^ m]
        s = t[:, 0]
        norm = s if mutation in ("squared_norm", "l1_norm") else np.sqrt(s)
        ok = (norm > 0) & np.isfinite(norm)
        out = np.zeros((n, pad4(k)))
        out[:, :k] = np.where(ok[:, None], M / norm[:, None], 0.0 if mutation == "zero_rows_are_zero" else np.nan)
    return out, norm


def lists_statement(R, k_top, metric, sel=None, include_self=False, mutation=None, order=None):
    """``(ids int32 [n, k_top], values [n, k_top])`` of recommend.neighbours among R's own rows on the
    host in float64: the statement's rows, the tile's sum with the factors in ``order``, the total
    order.  ``mutation``: self_not_excluded; sigmoid_values (the values go through the sigmoid)."""
    assert mutation is None or mutation in LIST_MUTATIONS
    R = np.asarray(R, dtype=np.float64)
    n, k = R.shape
    rows_ = normalise_statement(R, k)[0][:, :k] if metric == "cosine" else R
    zero = np.zeros(n)
    with np.errstate(all="ignore"):
        z = pc.pair_float64(rows_, zero, rows_, zero, 0.0, order)
    sel = np.arange(n) if sel is None else np.asarray(sel)
    ids = np.full((len(sel), k_top), -1, dtype=np.int32)
    values = np.full((len(sel), k_top), np.nan)
    for s, q in enumerate(sel):
        cand = ~np.isnan(z[q])
        if not include_self and mutation != "self_not_excluded":
            cand[q] = False
        idx = np.flatnonzero(cand)
        best = idx[np.lexsort((-idx, -z[q][idx]))][:k_top]
        ids[s, :len(best)], values[s, :len(best)] = best, z[q][best]
    if mutation == "sigmoid_values":
        values = pc.sigmoid64(values)
    return ids, values


# --------------------------------------------------------------------------
# the checks that the GPU tests and the mutation tests share
# --------------------------------------------------------------------------
def assert_normalised(out, norm, R, k, what):
    """Normalised rows and norms against the long-double oracle at the element bound; NaN rows where
    the oracle has none to give; the padding exactly +0.0."""
    out, norm = np.asarray(out), np.asarray(norm)
    want_norm, want = norms_ld(R)
    assert out.shape == (np.asarray(R).shape[0], pad4(k)), (what, out.shape)
    E = LD(element_bound(k))
    pc.assert_within(out[:, :k], want, E * np.abs(want), f"{what} rows")
    defined = ~np.isnan(want).any(axis=1)
    pc.assert_within(norm[defined], want_norm[defined], E * want_norm[defined], f"{what} norms")
    pad = out[:, k:]
    assert not pad.any() and not np.signbit(pad).any(), f"{what}: the padding is not +0.0"


def assert_lists(ids, values, o, k_top, sel=None, excluded=None, what=""):
    """Lists against the oracle ``o``: the oracle's id at every separated position, every value within
    its derived tolerance of the oracle's value for the id returned, no id twice, none that
    ``excluded`` (bool [rows of o, candidates]) names, pads of id -1 / value NaN and nothing else
    after a query's last candidate."""
    ids, values = np.asarray(ids), np.asarray(values)
    sel = np.arange(o.z.shape[0]) if sel is None else np.asarray(sel)
    want, sep, n_ranked = pc.oracle_lists(o, k_top, sel, excluded)
    assert ids.shape == want.shape == values.shape, (what, ids.shape, want.shape, values.shape)
    wrong = (ids != want) & sep
    assert not wrong.any(), (f"{what}: {int(wrong.sum())} separated positions differ; first at "
                             f"{tuple(np.argwhere(wrong)[0])}: got {ids[wrong][0]}, want {want[wrong][0]}")
    filled = np.arange(k_top)[None, :] < np.minimum(n_ranked, k_top)[:, None]
    assert ((ids >= 0) == filled).all() and (ids[~filled] == -1).all(), f"{what}: the pads are not where they belong"
    assert np.isnan(values[~filled]).all(), f"{what}: a pad's value is not NaN"
    for s, q in enumerate(sel):
        got = ids[s][filled[s]]
        assert got.max(initial=-1) < o.z.shape[1] and len(set(got.tolist())) == got.size, f"{what}: query {q} repeats an id"
        if excluded is not None:
            assert not excluded[q][got].any(), f"{what}: query {q} was given an excluded id"
    col = np.where(filled, ids, 0)
    want_z = np.where(filled, o.z[sel[:, None], col], LD(np.nan))
    tol = np.where(filled, o.tol_z[sel[:, None], col], LD(0))
    return pc.assert_within(values, want_z, tol, f"{what} values")


# --------------------------------------------------------------------------
# the raw ABI calls
# --------------------------------------------------------------------------
def normalise(rfm, M, k, n_rows=None, ld=None):
    """rfm_rows_normalise of the first ``n_rows`` rows of ``M [n, k]`` stored with row stride ``ld``
    (default k) into sentinel-filled buffers of all its rows and a guard -> (out [n, kpad], norm [n])
    as the call left them, after the check that nothing behind the launch's rows was written."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    rt = rfm[3]
    M = np.asarray(M, dtype=np.float64)
    n, kpad = M.shape[0], pad4(k)
    n_rows, ld = n if n_rows is None else n_rows, k if ld is None else ld
    stored = np.full((n, ld), 123.456)  # (what lies between the rows must not matter)
    stored[:, :k] = M
    d_M = rt.upload(stored)
    out = pc._filled(rt, (n * kpad + pc.GUARD,), torch.float64)
    norm = pc._filled(rt, (n + pc.GUARD,), torch.float64)
    _lib.check(rt.lib.rfm_rows_normalise(rt.ctx, d_M.data_ptr(), n_rows, k, ld, out.data_ptr(), norm.data_ptr()))
    rt.sync()
    out, norm = out.cpu().numpy(), norm.cpu().numpy()
    assert (out[n_rows * kpad:].view(np.int64) == pc.SENTINEL_F64.view(np.int64)).all(), "d_out was written past its rows"
    assert (norm[n_rows:].view(np.int64) == pc.SENTINEL_F64.view(np.int64)).all(), "d_norm was written past its rows"
    return out[:n * kpad].reshape(n, kpad), norm[:n]


def topk_raw(rfm, A, LU, B, LI, c, K, user_ids=None, excl=None):
    """rfm_pair_topk_raw with test_gpu_recommend._abi_topk's argument handling, into sentinel-filled
    outputs -> (items, values)."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    _, _, recommend, rt = rfm
    A, LU, B, LI = pc._own(A, LU, B, LI)
    kf = A.shape[1]
    dA, dB = rt.upload(pc._padded(A)), rt.upload(pc._padded(B))
    dLU, dLI, dc = rt.upload(LU), rt.upload(LI), rt.upload(np.array([c], dtype=np.float64))
    ids = None if user_ids is None else rt.upload(np.asarray(user_ids, dtype=np.int32))
    n_sel = A.shape[0] if user_ids is None else len(user_ids)
    ws = rt.empty((recommend.topk_workspace_bytes(n_sel, B.shape[0], K),), torch.uint8)
    items = pc._filled(rt, (n_sel, K), torch.int32)
    values = pc._filled(rt, (n_sel, K), torch.float64)
    ex = (None, None) if excl is None else (rt.upload(excl[0].astype(np.int64)), rt.upload(excl[1].astype(np.int32)))
    _lib.check(rt.lib.rfm_pair_topk_raw(
        rt.ctx, dA.data_ptr(), dLU.data_ptr(), A.shape[0], None if ids is None else ids.data_ptr(), n_sel,
        dB.data_ptr(), dLI.data_ptr(), B.shape[0], kf, dc.data_ptr(), None if ex[0] is None else ex[0].data_ptr(),
        None if ex[1] is None else ex[1].data_ptr(), K, ws.data_ptr(), items.data_ptr(), values.data_ptr()))
    rt.sync()
    got = items.cpu().numpy(), values.cpu().numpy()
    pc.assert_written(*got)
    return got
