"""Shared by the diversified re-ranking tests (test_diverse_host.py, test_gpu_diverse.py,
test_gpu_diverse_models.py; rfm_diverse_select of csrc/rfm_diverse.hip, recommend.diversify / diverse,
DESIGN.md 8 N24): a NumPy float64 statement of the whole selection with every sum in the order
include/rfm_diverse.h states (it carries six mutations), a long-double oracle with derived tolerances
and the separation of every step, an independent plain NumPy MMR, the case lists, the checkers that
both the GPU tests and the mutation tests go through, and the raw ABI call.  Importing this module
touches neither the GPU nor the package under test.

With u = 2^-53 and c = ceil(n_factors / 64), the trips of a lane's factor loop:

sim     every term is a rounded product (1 u) and goes through at most c adds of its lane (the first,
        to +0.0, is exact) and the 6 adds of the xor tree: |d sim| <= (c + 7) u S (times 1 + 2^-40 for
        the second-order terms), S = sum_f |x_f y_f| -- the summation depth that
        neighbours_common.element_bound counts for the same tree.  The rows are INPUTS here: the
        oracle takes the float64 rows the kernel takes, so no normalisation error enters.
m       the maximum of similarities each within its tolerance is within the largest of them.
value   lambda and r = fl(1 - lambda) are the formula's coefficients (the header: "1 - lambda one
        double subtraction"), so the oracle uses the same r.  v = (lambda p [- penalty]) - r m has one
        rounding per operation -- the product lambda p, the product r m, the difference; a fourth,
        the penalty's subtraction, where a penalty is given:
        |d v| <= u (|lambda p| [+ |base|] + |r m| + |v|) (1 + 2^-40) + r tol_m.
        Step 0 is held to the same expression with its m term zero, u (|lambda p| [+ |base|] + |v|):
        a bound still (the difference it counts is not formed there), and one that leaves the floor
        below room -- a single rounding can come as close to u |x| as it likes.

A step is SEPARATED when the oracle's best eligible candidate b beats every other eligible
candidate c by more than the two tolerances together, v_b - v_c > tol_b + tol_c (twice the
tolerance where they are equal): then every computation within the tolerances makes the same pick.
The random case lists are chosen so that EVERY step of every list is separated (test_diverse_host.py
asserts the share 1.0); exact ties are planted cases of their own and are held bitwise only.

All derived, none measured."""
import ctypes
import functools
import types

import numpy as np

import neighbours_common as nc
import pair_tile_common as pc
from pair_tile_common import LD, U, pad4

LANES = 64
SECOND_ORDER = 1.0 + 2.0 ** -40
MAX_DEPTH, MAX_K = 1024, 64
BLOCK = 256  # threads of a workgroup: candidates per pass of the value loop
MUTATIONS = ("mean_similarity", "stale_maximum", "ties_to_lower_id", "nan_similarity_ineligible", "penalty_added",
             "drops_last_factor")
GEOMETRY_NAMES = ("form", "workgroups", "passes", "candidates_per_thread", "lds_bytes", "factor_trips")

# the host's case lists (the issue's): 4 lists, 64 steps
HOST_FACTORS = (1, 2, 5, 37, 400)
HOST_DEPTHS = (65, 257, 1024)
HOST_LAMBDAS = (0.3, 0.7)
# the GPU's: the edges of the lane loop, the thread stride and the grid
GPU_FACTORS = (1, 2, 5, 37, 63, 64, 65, 128, 129, 400, 1024)
GPU_DEPTHS = (1, 2, 63, 64, 65, 255, 256, 257, 1023, 1024)
GPU_DEPTH_FACTORS = (5, 37)
GPU_K = (1, 2, 9, 64)
GPU_LAMBDAS = (0.0, 0.3, 0.7, 1.0)
GPU_LISTS = 3


# --------------------------------------------------------------------------
# inputs
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(n_lists, depth, kf, seed=0):
    """A random case: ``n_items = depth + 9`` normalised rows ~ N(0, 1) (the float64 statement of
    rfm_rows_normalise: what the device hands the selection), per list ``depth`` distinct items in
    random order with scores the sorted (descending) sigmoid of N(0, 1.5), and a penalty ~ U(0, 0.2)
    per item.  Computed once, shared, read-only."""
    rng = np.random.default_rng([n_lists, depth, kf, seed, 24])
    n_items = depth + 9
    R = nc.normalise_statement(nc.rows(n_items, kf, seed), kf)[0][:, :kf].copy()
    items = np.stack([rng.permutation(n_items)[:depth] for _ in range(n_lists)]).astype(np.int32)
    scores = -np.sort(-pc.sigmoid64(1.5 * rng.standard_normal((n_lists, depth))), axis=1)
    penalty = 0.2 * rng.random(n_items)
    for a in (R, items, scores, penalty):
        a.setflags(write=False)
    return types.SimpleNamespace(items=items, scores=scores, R=R, penalty=penalty, n_items=n_items, kf=kf,
                                 depth=depth, n_lists=n_lists)


def random_gpu_cases():
    """``(name, (n_lists, depth, kf), k)`` of every random case of test_gpu_diverse.py: the factor counts at
    depth 65, the depths at 5 and 37 factors, the pick counts -- k = 64 of 63 candidates pads."""
    out = [(f"factors={kf}", (GPU_LISTS, 65, kf), 9) for kf in GPU_FACTORS]
    out += [(f"depth={depth} factors={kf}", (GPU_LISTS, depth, kf), 9) for depth in GPU_DEPTHS for kf in GPU_DEPTH_FACTORS]
    out += [(f"k={k}", (GPU_LISTS, 65, 37), k) for k in GPU_K] + [("k=64 of 63", (GPU_LISTS, 63, 5), 64)]
    return out


def special_case(kf=5):
    """One list of 65 candidates over 80 items with every special input at once, and what to expect of it:
    a NaN row (item 70) and an Inf row (item 71) with the two highest scores, so that both are chosen
    and every other candidate meets them as the chosen item; ids outside the table (-7, 83, 2^31 - 1);
    a NaN score on a valid id; a repeated id (item 12 at positions 5 and 9, the same score); the tail
    padded with item -1 / score NaN as rfm_pair_order pads."""
    rng = np.random.default_rng(kf + 1000)
    n_items, depth = 80, 65
    R = nc.normalise_statement(nc.rows(n_items, kf, 3), kf)[0][:, :kf].copy()
    R[70] = np.nan
    R[71] = 0.25
    R[71, kf - 1] = np.inf
    items = rng.permutation(60)[:depth - 5].astype(np.int32)  # 60 candidates among items 0 .. 59
    items = np.concatenate([items, np.full(5, -1, np.int32)])
    scores = np.concatenate([-np.sort(-pc.sigmoid64(1.5 * rng.standard_normal(depth - 5))), np.full(5, np.nan)])
    items[0], items[1] = 70, 71
    items[3], items[20], items[33] = -7, 83, 2 ** 31 - 1
    scores[15] = np.nan
    items[5] = items[9] = 12
    scores[9] = scores[5]
    where = dict(nan_row=0, inf_row=1, outside=(3, 20, 33), nan_score=15, repeat=(5, 9), padded=tuple(range(60, 65)))
    return types.SimpleNamespace(items=items[None, :], scores=scores[None, :], R=R, penalty=0.2 * rng.random(n_items),
                                 n_items=n_items, kf=kf, depth=depth, n_lists=1, where=where)


def twin_case(kf=5):
    """Three lists over 39 items in which items 7 and 31 have the same row and, in every list, the same
    score (the list's highest): the two tie exactly at every step until one of them is chosen."""
    base = case(3, 30, kf, 5)
    R = base.R.copy()
    R[31] = R[7]
    items, scores = base.items.copy(), base.scores.copy()
    others = np.array([c for c in range(base.n_items) if c not in (7, 31)])
    for l in range(3):
        row = np.random.default_rng(l).permutation(others)[:30]
        row[2], row[11] = 7, 31
        items[l] = row
        scores[l, 2] = scores[l, 11] = scores[l, 0] + 0.01
    return types.SimpleNamespace(items=items, scores=scores, R=R, penalty=base.penalty.copy(), n_items=base.n_items,
                                 kf=kf, depth=30, n_lists=3, twins=(7, 31))


# --------------------------------------------------------------------------
# the float64 statement of the kernel
# --------------------------------------------------------------------------
def sims_statement(C, y, kf, drop_last=False):
    """``[n]``: the dot products of the rows ``C [n, >= kf]`` with ``y`` over f < kf in the header's
    order -- lane l starts from +0.0 and adds the rounded products of the factors l, l + 64, ...
    ascending; the 64 sums go through the xor tree m = 32 .. 1 (neighbours_common.normalise_statement's
    machinery).  ``drop_last``: at kf % 64 == 1 the last factor is left out."""
    C, y = np.asarray(C, dtype=np.float64)[:, :kf], np.asarray(y, dtype=np.float64)[:kf]
    n, chunks = C.shape[0], -(-kf // LANES)
    with np.errstate(all="ignore"):
        P = np.zeros((n, chunks * LANES))  # (a lane without a factor adds +0.0, which changes no bit of its sum)
        P[:, :kf] = C * y[None, :]
        if drop_last and kf % LANES == 1:
            P[:, kf - 1] = 0.0
        t = np.zeros((n, LANES))
        for j in range(chunks):
            t = t + P[:, LANES * j: LANES * (j + 1)]
        lane = np.arange(LANES)
        for m in (32, 16, 8, 4, 2, 1):
            t = t + t[:, lane ^ m]
    return t[:, 0]


def _best(v, items, idx, low_id=False):
    """Of the eligible positions ``idx`` the best: value descending, item id descending, position ascending."""
    order = np.lexsort((idx, items[idx] if low_id else -items[idx].astype(np.int64), -v[idx]))
    return idx[order]


def select_statement(items, scores, R, kf, penalty, lam, k, mutation=None):
    """``(items int32, scores, values, pos int32)``, each ``[n_lists, k]``: rfm_diverse_select in float64,
    operation by operation as include/rfm_diverse.h orders them.  ``R`` is ``[n_items, >= kf]`` (the
    row stride plays no part in the arithmetic), ``penalty`` ``[n_items]`` or None.  ``mutation``:

    - mean_similarity: m is the mean of the similarities to the picks so far, not their maximum;
    - stale_maximum: the maximum leaves out the most recent pick (before the second pick: no term);
    - ties_to_lower_id: equal values go to the lower item id;
    - nan_similarity_ineligible: a candidate whose similarity to a pick is NaN is never chosen;
    - penalty_added: the penalty is added;
    - drops_last_factor: at kf % 64 == 1 the dot products leave out the last factor."""
    assert mutation is None or mutation in MUTATIONS
    items, scores = np.asarray(items), np.asarray(scores, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)
    n_lists, depth = items.shape
    n_items = R.shape[0]
    lam = np.float64(lam)
    rest = np.float64(1.0) - lam
    out_items, out_pos = np.full((n_lists, k), -1, np.int32), np.full((n_lists, k), -1, np.int32)
    out_scores, out_values = np.full((n_lists, k), np.nan), np.full((n_lists, k), np.nan)
    with np.errstate(all="ignore"):
        for l in range(n_lists):
            it, p = items[l].astype(np.int64), scores[l]
            ok = (it >= 0) & (it < n_items) & ~np.isnan(p)
            row = np.where(ok, it, 0)
            base = lam * p
            if penalty is not None:
                pen = np.asarray(penalty, dtype=np.float64)[row]
                base = np.where(ok, base + pen if mutation == "penalty_added" else base - pen, base)
            m = np.full(depth, -np.inf)
            total, last = np.zeros(depth), None
            for t in range(k):
                if t == 0:
                    v = base
                elif mutation == "mean_similarity":
                    v = base - rest * (total / t)
                elif mutation == "stale_maximum":
                    v = base - rest * np.where(np.isinf(m), 0.0, m)
                else:
                    v = base - rest * m
                idx = np.flatnonzero(ok & ~np.isnan(v))
                if not idx.size:
                    break
                b = _best(v, it, idx, mutation == "ties_to_lower_id")[0]
                out_items[l, t], out_scores[l, t], out_values[l, t], out_pos[l, t] = it[b], p[b], v[b], b
                ok[b] = False
                if t + 1 == k:
                    break
                s = sims_statement(R[row], R[it[b]], kf, mutation == "drops_last_factor")
                if mutation == "nan_similarity_ineligible":
                    ok &= ~np.isnan(s)
                s = np.where(np.isnan(s), 0.0, s)
                total = total + s
                if mutation == "stale_maximum":
                    if last is not None:
                        m = np.where(last > m, last, m)
                    last = s
                else:
                    m = np.where(s > m, s, m)
    return out_items, out_scores, out_values, out_pos


# --------------------------------------------------------------------------
# the long-double oracle and an independent plain MMR
# --------------------------------------------------------------------------
def select_oracle(items, scores, R, kf, penalty, lam, k):
    """The selection in np.longdouble -> namespace of ``items``, ``pos`` (int, -1 = none), ``values``
    (LD), ``tol`` (LD: the chosen value's tolerance), ``separated`` (bool) -- each ``[n_lists, k]`` --
    and ``gap``, the smallest margin v_b - v_c - tol_b - tol_c of any step (module docstring)."""
    items, scores = np.asarray(items), np.asarray(scores, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)[:, :kf]
    n_lists, depth = items.shape
    n_items = R.shape[0]
    Rl, Ra = R.astype(LD), np.abs(R).astype(LD)
    u, so = LD(U), LD(SECOND_ORDER)
    D = LD(-(-kf // LANES) + 7)
    lam_l, rest = LD(np.float64(lam)), LD(np.float64(1.0) - np.float64(lam))
    o = types.SimpleNamespace(items=np.full((n_lists, k), -1, np.int64), pos=np.full((n_lists, k), -1, np.int64),
                              values=np.full((n_lists, k), np.nan, LD), tol=np.zeros((n_lists, k), LD),
                              separated=np.ones((n_lists, k), bool), gap=np.inf)
    with np.errstate(all="ignore"):
        for l in range(n_lists):
            it, p = items[l].astype(np.int64), scores[l]
            ok = (it >= 0) & (it < n_items) & ~np.isnan(p)
            row = np.where(ok, it, 0)
            lp = lam_l * p.astype(LD)
            base, tol_base = lp, u * np.abs(lp)
            if penalty is not None:
                base = lp - np.asarray(penalty, dtype=np.float64)[row].astype(LD)
                tol_base = tol_base + u * np.abs(base)
            C, Ca = Rl[row], Ra[row]
            m, tol_m = np.full(depth, -np.inf, LD), np.zeros(depth, LD)
            for t in range(k):
                if t == 0:
                    v, tol = base, (tol_base + u * np.abs(base)) * so  # (the formula's bound with its m term zero)
                else:
                    w = rest * m
                    v = base - w
                    tol = (tol_base + u * (np.abs(w) + np.abs(v))) * so + rest * tol_m
                idx = np.flatnonzero(ok & ~np.isnan(v))
                if not idx.size:
                    break
                ranked = _best(v, it, idx)
                b = ranked[0]
                if ranked.size > 1:
                    others = ranked[1:]
                    margin = np.min(v[b] - v[others] - tol[b] - tol[others])
                    o.separated[l, t] = bool(margin > 0)
                    o.gap = min(o.gap, float(margin))
                o.items[l, t], o.pos[l, t], o.values[l, t], o.tol[l, t] = it[b], b, v[b], tol[b]
                ok[b] = False
                s, S = C @ Rl[it[b]], Ca @ Ra[it[b]]
                tol_s = np.where(np.isnan(s), LD(0), D * u * S * so)
                s = np.where(np.isnan(s), LD(0), s)
                m, tol_m = np.where(s > m, s, m), np.maximum(tol_m, tol_s)
    return o


def plain_mmr(items, scores, R, kf, penalty, lam, k):
    """``(items, pos)`` ``[n_lists, k]`` of textbook MMR in float64: the full Gram matrix of a list's
    candidates, a Python list of picks, ``argmax``.  Valid inputs only (ids inside the table, no NaN)."""
    items, scores = np.asarray(items), np.asarray(scores, dtype=np.float64)
    R = np.asarray(R, dtype=np.float64)[:, :kf]
    out_items, out_pos = np.full((items.shape[0], k), -1, np.int64), np.full((items.shape[0], k), -1, np.int64)
    for l in range(items.shape[0]):
        G = R[items[l]] @ R[items[l]].T
        relevance = lam * scores[l] - (0.0 if penalty is None else np.asarray(penalty)[items[l]])
        picks = []
        for t in range(min(k, items.shape[1])):
            redundancy = G[:, picks].max(axis=1) if picks else np.zeros(len(relevance))
            value = relevance - (1.0 - lam) * redundancy
            value[picks] = -np.inf
            picks.append(int(np.argmax(value)))
        out_pos[l, :len(picks)], out_items[l, :len(picks)] = picks, items[l][picks]
    return out_items, out_pos


# --------------------------------------------------------------------------
# the checks that the GPU tests and the mutation tests share
# --------------------------------------------------------------------------
def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def assert_same_bits(got, want, what, lists=None):
    """The four outputs ``got`` against the statement's ``want`` byte for byte (a NaN may be any NaN);
    ``lists``: only these rows."""
    for name, g, w in zip(("items", "scores", "values", "pos"), got, want):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        if lists is not None:
            g, w = g[lists], w[lists]
        if g.dtype == np.float64:
            nan = np.isnan(w)
            assert (np.isnan(g) == nan).all(), f"{what} {name}: NaN where a number belongs, or the reverse"
            differ = (_bits(g) != _bits(w)) & ~nan
        else:
            differ = g != w
        assert not differ.any(), (f"{what} {name}: {int(differ.sum())} of {differ.size} elements differ; first at "
                                  f"{tuple(np.argwhere(differ)[0])}: got {g[differ][0]!r}, want {w[differ][0]!r}")


def assert_against_oracle(got, o, scores, what, lists=None, bound=1.0):
    """The four outputs against the oracle ``o``: at every step up to a list's first unseparated one the
    oracle's item and position, the candidate's score byte for byte, the value within its tolerance;
    pads of -1 / NaN / NaN / -1 and nothing else once the oracle has no candidate left.  Returns the
    largest |d value| / tol."""
    g_items, g_scores, g_values, g_pos = (np.asarray(a) for a in got)
    scores = np.asarray(scores, dtype=np.float64)
    worst = 0.0
    for l in (range(o.items.shape[0]) if lists is None else lists):
        for t in range(o.items.shape[1]):
            if o.pos[l, t] < 0:
                assert (g_items[l, t:] == -1).all() and (g_pos[l, t:] == -1).all(), f"{what}: list {l} pads from step {t}"
                assert np.isnan(g_scores[l, t:]).all() and np.isnan(g_values[l, t:]).all(), f"{what}: list {l} pads"
                break
            if not o.separated[l, t]:
                break  # (from here on two correct computations may hold different lists)
            assert g_items[l, t] == o.items[l, t] and g_pos[l, t] == o.pos[l, t], (
                f"{what}: list {l} step {t}: got item {g_items[l, t]} at {g_pos[l, t]}, want {o.items[l, t]} at {o.pos[l, t]}")
            assert _bits(g_scores[l, t:t + 1])[0] == _bits(scores[l, o.pos[l, t]:o.pos[l, t] + 1])[0], (
                f"{what}: list {l} step {t}: the score is not the candidate's")
            ex = float(pc.excess(g_values[l, t:t + 1], o.values[l, t:t + 1], o.tol[l, t:t + 1])[0])
            assert ex <= bound, (f"{what}: list {l} step {t}: value {g_values[l, t]!r}, want {float(o.values[l, t])!r}, "
                               f"|d| / tol {ex!r}")
            worst = max(worst, ex)
    print(f"{what}: largest |d value| / tol {worst:.3g}")
    return worst


def refuses(check, *args, **kwargs):
    try:
        check(*args, **kwargs)
    except AssertionError:
        return True
    return False


# --------------------------------------------------------------------------
# the raw ABI calls
# --------------------------------------------------------------------------
def geometry(n_lists, depth, kf, ld_R=None, k=9, ctx=None):
    """rfm_diverse_geometry (host only; ``ctx`` None: a device of 256 CUs) -> dict of GEOMETRY_NAMES."""
    from relevance_factorizationmachine_amd import _lib
    out = np.full(6, -1, dtype=np.int64)
    _lib.check(_lib.load().rfm_diverse_geometry(ctx, int(n_lists), int(depth), int(kf), int(kf if ld_R is None else ld_R),
                                                int(k), out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))))
    return dict(zip(GEOMETRY_NAMES, (int(v) for v in out)))


def select(rfm, items, scores, R, kf, penalty, lam, k, ld_c=None, ld_R=None, expect=0):
    """rfm_diverse_select on ``items, scores [n_lists, depth]`` stored with row stride ``ld_c`` and rows
    ``R [n_items, kf]`` stored with stride ``ld_R`` into sentinel-filled outputs with a guard behind
    each -> the four outputs ``[n_lists, k]``, after the checks that the call returned ``expect`` and
    that nothing behind an output was written.  A refused call (``expect`` != 0) must leave every
    output byte as it was."""
    import torch
    rt = rfm[3]
    items, scores = np.asarray(items, dtype=np.int32), np.asarray(scores, dtype=np.float64)
    n_lists, depth = items.shape
    ld_c, ld_R = depth if ld_c is None else ld_c, kf if ld_R is None else ld_R
    h_items, h_scores = np.full((n_lists, max(ld_c, 1)), 12345, np.int32), np.full((n_lists, max(ld_c, 1)), 0.5)
    if ld_c >= depth:  # (what lies between the rows must not matter)
        h_items[:, :depth], h_scores[:, :depth] = items, scores
    R = np.asarray(R, dtype=np.float64)
    h_R, w = np.full((R.shape[0], max(ld_R, kf, 1)), 123.456), min(max(kf, 0), R.shape[1])
    h_R[:, :w] = R[:, :w]
    d = [rt.upload(a) for a in (h_items, h_scores, h_R)]
    d_pen = None if penalty is None else rt.upload(np.array(penalty, dtype=np.float64))
    n_out = n_lists * max(k, 1) if 1 <= k <= MAX_K else n_lists
    outs = [pc._filled(rt, (n_out + pc.GUARD,), dt) for dt in (torch.int32, torch.float64, torch.float64, torch.int32)]
    rc = rt.lib.rfm_diverse_select(rt.ctx, d[0].data_ptr(), d[1].data_ptr(), n_lists, depth, ld_c, d[2].data_ptr(),
                                   R.shape[0], kf, ld_R, None if d_pen is None else d_pen.data_ptr(), float(lam), k,
                                   *(t.data_ptr() for t in outs))
    rt.sync()
    assert rc == expect, (rc, expect)
    got = [t.cpu().numpy() for t in outs]
    written = 0 if expect else n_out
    for a in got:
        sentinel = pc.SENTINEL_I32 if a.dtype == np.int32 else pc.SENTINEL_F64
        assert (_bits(a[written:]) == _bits(np.array([sentinel]))[0]).all(), "an output was written where it must not be"
    if expect:
        return None
    got = tuple(a[:n_out].reshape(n_lists, k) for a in got)
    for a in (got[0], got[3]):
        assert not (a == pc.SENTINEL_I32).any(), "an output element was not written"
    for a in (got[1], got[2]):
        assert not (_bits(a) == _bits(np.array([pc.SENTINEL_F64]))[0]).any(), "an output element was not written"
    return got
