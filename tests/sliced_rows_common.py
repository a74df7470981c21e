"""Shared by the row-by-row tests of the sliced FM forward (fm_logit_slices_kernel, rfm_fm_sliced.hpp:
test_sliced_oracle_host.py, test_gpu_sliced_rows.py): logs whose rows hold a CHOSEN number of cached
and uncached entries, training logs whose cached columns and their LDS order are known beforehand,
a float64 statement of the kernel's arithmetic with four mutations, the plan's slice table, and thin
wrappers of rfm_fm_plan_forward and the host-only queries.  The oracle, the tolerances and the
parameters are forward_rows_common's, unchanged.  Importing this module touches neither the GPU nor
the package under test.

Columns.  ``columns(F, R)``: F "frequent" and R "rare" columns interleaved in index (while both kinds
last, every third index is a frequent one), so that a sorted row alternates between the kinds and the
translation has to move the cached entries to the front.  The frequent columns' counts in a training
log are distinct, at least 1/16 of the rows and dealt to the columns in a shuffled order: the plan's
cached columns (at least one row in 64) and their LDS order (descending count) are ``freq`` itself,
cut at the LDS cap.  A rare column is in at most 1/256 of the rows.

The class log (``class_log``) of ML records per row, nh cached and ng uncached entries in a row:
  - four times each (nh, ng) of nh in {0, 1, 2, 3, 4, 5, 7, 8, 9} x ng in {0 .. 5} (around the
    batches of kSlBatch = 4 cached entries and the kSlGlobals = 2 gathers requested a row ahead);
  - twice the full rows (ML, 0), (0, ML), (ML - 1, 1), (ML - 3, 3);
  - twice each long row of ML + 1, 65, 128, 129 entries: mixed, uncached-only and -- where the 64
    frequent columns suffice, a row names a column once -- cached-only (ML = 16: 17, ML = 32: 33;
    test_gpu_sliced_rows.py part B scores cached-only rows of 65, 128 and 129 entries on the logs
    that have that many cached columns);
  - empty rows, the first and the last row among them;
  - a strip of 91 rows whose kinds (empty, long, cached-only, more than two uncached, mixed) have
    the period 25 and follow, 16 rows apart, a cycle through all 25 ordered pairs of kinds: every
    ordered pair sits at r, r + 25 and r + 50 for some r, so a workgroup of 41 rows or more has one
    of them inside (``pairs_inside``; the device test asserts it from the queried rows per workgroup).
All at shuffled positions (the strip in one piece)."""
import functools

import numpy as np
from scipy.sparse import csr_matrix

import forward_rows_common as fr

LD = np.longdouble
N_FREQ, N_RARE = 64, 134          # the class logs' columns: a row of 129 uncached entries fits
TRAIN_ROWS = 2000
PARAM_LPR = 32                    # forward_params: the pair term's deviation is about 3 at 65 entries
KINDS = ("empty", "long", "cached-only", "more than two uncached", "mixed")
NH_GRID, NG_GRID = (0, 1, 2, 3, 4, 5, 7, 8, 9), (0, 1, 2, 3, 4, 5)
# the plan's slices (rfm_fm_plan.hip): k -> (slices, factors per slice, width of the last slice)
SLICE_TABLE = {130: (1, 130, 130), 256: (1, 256, 256), 258: (2, 130, 128), 384: (2, 192, 192),
               512: (2, 256, 256), 514: (4, 130, 124), 1022: (4, 256, 254), 1024: (4, 256, 256)}


def slices_of(k):
    """The plan's formula: one slice per 256 factors rounded up to a power of two, evenly wide, even."""
    ns = 1
    while ns * 256 < k:
        ns *= 2
    sw = ((k + ns - 1) // ns + 1) & ~1
    return ns, sw, k - (ns - 1) * sw


def lds_cap(sw):
    """Cached columns that fit: 160 KiB of LDS less 2 KiB readable past the last row and 1 KiB kept
    back, rows of sw doubles + a norm + 8 bytes of padding, one of them the row of zeros."""
    return ((160 << 10) - 2048 - 1024) // (8 * sw + 16) - 1


# --------------------------------------------------------------------------
# columns and training logs
# --------------------------------------------------------------------------
class Columns:
    def __init__(self, F, R, seed=0):
        self.F, self.R, self.n = F, R, F + R
        kind = np.zeros(self.n, dtype=bool)       # True: frequent
        m = min(F, R // 2)                        # interleaved while both kinds last
        kind[1: 3 * m: 3] = True
        rest = np.flatnonzero(~kind)[::-1][: F - m]   # (more frequent than rare ones: from the back)
        kind[rest] = True
        assert kind.sum() == F
        rng = np.random.default_rng(1000 + 7 * F + seed)
        self.freq = rng.permutation(np.flatnonzero(kind)).astype(np.int32)   # by descending count
        self.rare = np.flatnonzero(~kind).astype(np.int32)


def _row(rng, cols):
    cols = np.sort(np.asarray(cols, dtype=np.int32))
    return cols, rng.standard_normal(len(cols))


def _csr(rows, n_cols):
    indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int64)
    cols = np.concatenate([c for c, _ in rows] + [np.zeros(0, np.int32)]).astype(np.int32)
    x = np.concatenate([v for _, v in rows] + [np.zeros(0)])
    return csr_matrix((x, cols, indptr), shape=(len(rows), n_cols))


def _labels(rng, n):
    return {"labels": (rng.random(n) < 0.5).astype(np.int64), "pscores": rng.uniform(0.1, 1.0, size=n) ** 0.5}


@functools.lru_cache(maxsize=None)
def train_log(F, R, max_len, long_rows=(), n_empty=0, n_rows=TRAIN_ROWS):
    """A training log of ``n_rows`` rows on Columns(F, R): frequent column of rank j in
    n_rows / 16 + 3 (F - 1 - j) of the ordinary rows (dealt round robin over a shuffle of them: a
    column's rows are distinct), each rare column in 4 of them; row 5 is filled with rare columns to
    ``max_len`` entries, the longest ordinary row; rows 7, 9, .. hold ``long_rows`` entries (half of
    them frequent columns, at most 60) and rows 6, 8, .. (``n_empty`` of them) are empty.  Returns
    (log, columns, the row numbers by name)."""
    C = Columns(F, R)
    rng = np.random.default_rng(50_000 + 131 * F + max_len)
    named = {"longest": 5, "long": [7 + 2 * i for i in range(len(long_rows))],
             "empty": [6 + 2 * i for i in range(n_empty)]}
    special = {named["longest"], *named["long"], *named["empty"]}
    ordinary = rng.permutation([r for r in range(n_rows) if r not in special])
    held = [[] for _ in range(n_rows)]
    at = 0
    for j, c in enumerate(C.freq):
        cnt = n_rows // 16 + 3 * (F - 1 - j)
        assert cnt < len(ordinary)
        for r in ordinary[(at + np.arange(cnt)) % len(ordinary)]:
            held[r].append(c)
        at += cnt
    for c in C.rare:
        for r in rng.choice(ordinary, size=4, replace=False):
            held[r].append(c)
    assert max(len(h) for h in held) < max_len <= R + F
    # (rare columns first; where they run out, frequent ones: a count moves by one, the order stays)
    fill = np.concatenate([rng.permutation(C.rare), rng.permutation(C.freq)])[:max_len]
    held[named["longest"]] = list(fill)
    for r, L in zip(named["long"], long_rows):
        nf = min(L // 2, 60, F)
        held[r] = list(rng.permutation(C.freq)[:nf]) + list(rng.permutation(C.rare)[: L - nf])
        assert len(held[r]) == L
    rows = [_row(rng, h) for h in held]
    X = _csr(rows, C.n)
    # what the plan will see: counts distinct and descending along freq, thresholds kept
    cnt = np.bincount(X.indices, minlength=C.n)
    if F:
        assert (np.diff(cnt[C.freq]) < 0).all() and cnt[C.freq].min() * 16 >= n_rows
    assert cnt[C.rare].max() * 256 <= n_rows
    assert np.diff(X.indptr).max() == max(max_len, *long_rows, 0)
    return dict(features=X, **_labels(rng, n_rows)), C, named


def records_per_row(longest_ordinary):
    ml = 16
    while ml < longest_ordinary and ml < 64:
        ml *= 2
    return ml


# --------------------------------------------------------------------------
# the class log
# --------------------------------------------------------------------------
def _pair_cycle():
    """e[0 .. 25): a cycle over the five kinds in which every ordered pair (self pairs too) is
    (e[i], e[i + 1]) once -- an Euler circuit of the complete digraph with loops."""
    out_edges = {a: list(range(5)) for a in range(5)}
    stack, circuit = [0], []
    while stack:
        v = stack[-1]
        if out_edges[v]:
            stack.append(out_edges[v].pop())
        else:
            circuit.append(stack.pop())
    e = circuit[::-1][:-1]
    assert len(e) == 25 and len({(e[i], e[(i + 1) % 25]) for i in range(25)}) == 25
    return e


def strip_kinds(length=91):
    """Kinds of the strip's rows: period 25, and the row 16 further on is the next of the cycle
    (c[16 i mod 25] = e[i]; 16 and 25 are coprime)."""
    e, c = _pair_cycle(), [0] * 25
    for i in range(25):
        c[16 * i % 25] = e[i]
    return [c[j % 25] for j in range(length)]


def kind_masks(nh, ng, ML):
    """Which of KINDS each row is (a row of four uncached entries and two cached ones is both mixed
    and of more than two uncached)."""
    L = nh + ng
    short = L <= ML
    return np.stack([L == 0, ~short, short & (nh > 0) & (ng == 0), short & (ng > 2), short & (nh > 0) & (ng > 0)])


def pairs_inside(masks, rows_per_wg, n_rows=None):
    """For every ordered pair of kinds: is there a row r of the first kind with r + 16 of the second,
    both below n_rows and in one workgroup's range?  -> bool [5, 5]"""
    n = masks.shape[1] if n_rows is None else n_rows
    r = np.arange(max(n - 16, 0))
    same = r // rows_per_wg == (r + 16) // rows_per_wg
    return np.array([[bool((masks[a, r] & masks[b, r + 16] & same).any()) for b in range(5)] for a in range(5)])


def _long_specs(ML):
    specs = []
    for L in sorted({ML + 1, 65, 128, 129}):
        specs.append((min(L // 2, 60), L - min(L // 2, 60)))   # mixed
        specs.append((0, L))                                   # uncached-only
        if L <= N_FREQ:
            specs.append((L, 0))                               # cached-only
    return specs


@functools.lru_cache(maxsize=None)
def class_log(ML, extra=0):
    """The class log of ``ML`` records per row on Columns(N_FREQ, N_RARE), ``extra`` more rows of
    random (nh, ng) from the grid appended before the last (empty) row -> (log, nh, ng) with the
    numbers of cached and uncached entries of every row."""
    C = Columns(N_FREQ, N_RARE)
    rng = np.random.default_rng(900 + ML)
    grid = [(h, g) for h in NH_GRID for g in NG_GRID if h + g <= ML]
    full = [(ML, 0), (0, ML), (ML - 1, 1), (ML - 3, 3)]
    longs = _long_specs(ML)
    loose = grid * 4 + full * 2 + longs * 2 + [(0, 0)] * 2
    loose = [loose[i] for i in rng.permutation(len(loose))]

    def of_kind(kind):
        if kind == 0:
            return 0, 0
        if kind == 1:
            return longs[rng.integers(len(longs))]
        if kind == 2:
            return int(rng.integers(1, 10)), 0
        if kind == 3:
            return int(rng.integers(0, 10)), int(rng.integers(3, 6))
        return int(rng.integers(1, 10)), int(rng.integers(1, 3))

    strip = [of_kind(kd) for kd in strip_kinds()]
    cut = len(loose) // 2
    more = [grid[i] for i in rng.integers(0, len(grid), size=extra)]
    spec = [(0, 0)] + loose[:cut] + strip + loose[cut:] + more + [(0, 0)]
    rows = [_row(rng, np.concatenate([rng.permutation(C.freq)[:h], rng.permutation(C.rare)[:g]])) for h, g in spec]
    nh, ng = np.array([h for h, _ in spec]), np.array([g for _, g in spec])
    return dict(features=_csr(rows, C.n), **_labels(rng, len(rows))), nh, ng


EDGE_RARE = 70   # rare columns of the cached-column logs of part B


@functools.lru_cache(maxsize=None)
def edge_log(F, H):
    """Evaluation rows for a training log of F frequent columns of which the first H (by rank) are
    cached.  The marked columns: the first cached one, the last, the one at rank 128 (the first of the
    second fill pass) and the first one cut off by the cap (rank H < F), where they exist.  Rows: each
    marked column alone, with one and with three rare columns; every pair of them; all together,
    bare and with rare columns; every cached column at once (a long row past 64 of them), also beside
    the cut column and rare ones; cached-only rows of 65, 128 and 129 entries where H allows; every
    frequent column; 40 rows of 0 .. 9 cached and 0 .. 5 other columns; the first, the last and two
    more rows empty.  -> (log, marked columns by name)"""
    C = Columns(F, EDGE_RARE)
    rng = np.random.default_rng(300 + F)
    ranks = {"first": 0, "last": H - 1, "rank 128": 128 if H > 128 else None, "cut": H if F > H else None}
    marked = {name: int(C.freq[r]) for name, r in ranks.items() if r is not None and 0 <= r < F}
    cols = list(dict.fromkeys(marked.values()))
    cached, other = C.freq[:H], np.concatenate([C.freq[H:], C.rare])

    def rare(m):
        return list(rng.permutation(C.rare)[:m])

    spec = [[]]
    for c in cols:
        spec += [[c], [c] + rare(1), [c] + rare(3)]
    spec += [[a, b] for i, a in enumerate(cols) for b in cols[i + 1:]]
    spec += [cols, cols + rare(3), [], list(cached), list(cached) + rare(2), list(C.freq), list(C.freq) + rare(5)]
    if "cut" in marked:
        spec += [list(cached) + [marked["cut"]], list(cached) + [marked["cut"]] + rare(3)]
    spec += [list(rng.permutation(cached)[:L]) for L in (65, 128, 129) if H >= L]
    for _ in range(40):
        spec.append(list(rng.permutation(cached)[: rng.integers(0, 10)]) + list(rng.permutation(other)[: rng.integers(0, 6)]))
    spec += [[], cols + rare(1), []]
    rows = [_row(rng, s) for s in spec]
    return dict(features=_csr(rows, C.n), **_labels(rng, len(rows))), marked


@functools.lru_cache(maxsize=None)
def theta(k, n_cols):
    """Parameters of a factor count and a column count (every log on those columns shares them)."""
    return fr.forward_params(2000 + k, n_cols, k, PARAM_LPR)


@functools.lru_cache(maxsize=None)
def class_case(ML, k, extra=0):
    """(class log, nh, ng, theta, oracle): computed once, shared, never modified."""
    log, nh, ng = class_log(ML, extra)
    th = theta(k, N_FREQ + N_RARE)
    return log, nh, ng, th, fr.row_oracle(log["features"], *th)


# --------------------------------------------------------------------------
# the kernel's arithmetic in float64
# --------------------------------------------------------------------------
def kernel_statement(X, w0, w, V, cached, k, shuffled=False, mutation=0, seed=0):
    """The sliced forward's sums in float64: per slice of the factors the cached entries first (their
    squares as x^2 |v_slice|^2 from a slice norm summed once per column), then the gathered entries
    with their own squares; slice 0 carries w0 + <w, x>; the slice partials added at the end; the
    clipped sigmoid.  ``cached``: the cached columns.  ``shuffled``: entries of a kind, the factors of
    a slice and the slices in another order.  ``mutation`` 1: without a row's 5th cached entry, 2: its
    3rd uncached one, 3: the last factor pair of the last slice, 4: x for x^2 in the square of a row's
    first cached entry."""
    ns, sw, _ = slices_of(k)
    rng = np.random.default_rng(seed)
    is_cached = np.zeros(X.shape[1], dtype=bool)
    is_cached[np.asarray(cached, dtype=np.int64)] = True
    bounds = [(s * sw, min((s + 1) * sw, k)) for s in range(ns)]
    if mutation == 3:
        bounds[-1] = (bounds[-1][0], k - 2)
    forder = [np.arange(a, b) for a, b in bounds]
    if shuffled:
        forder = [rng.permutation(f) for f in forder]
    norm = np.stack([(V[:, f] ** 2).sum(axis=1) for f in forder], axis=1)   # [n, ns]
    z = np.empty(X.shape[0])
    for r in range(X.shape[0]):
        cols, x = X.indices[X.indptr[r]: X.indptr[r + 1]], X.data[X.indptr[r]: X.indptr[r + 1]]
        hot = is_cached[cols]
        ch, xh, cg, xg = cols[hot], x[hot], cols[~hot], x[~hot]
        if shuffled:
            ph, pg = rng.permutation(len(ch)), rng.permutation(len(cg))
            ch, xh, cg, xg = ch[ph], xh[ph], cg[pg], xg[pg]
        if mutation == 1 and len(ch) >= 5:
            ch, xh = np.delete(ch, 4), np.delete(xh, 4)
        if mutation == 2 and len(cg) >= 3:
            cg, xg = np.delete(cg, 2), np.delete(xg, 2)
        xsq = xh * xh
        if mutation == 4 and len(ch):
            xsq = xsq.copy()
            xsq[0] = xh[0]
        parts = []
        for s, f in enumerate(forder):
            q = np.zeros(len(f))
            for c, xe in zip(ch, xh):
                q = q + V[c, f] * xe
            hn = float((xsq * norm[ch, s]).sum())
            s2 = np.zeros(len(f))
            for c, xe in zip(cg, xg):
                t = V[c, f] * xe
                q, s2 = q + t, s2 + t * t
            part = 0.5 * ((q * q - s2).sum() - hn)
            if s == 0:
                part = part + float((w[ch] * xh).sum() + (w[cg] * xg).sum()) + float(np.asarray(w0).reshape(-1)[0])
            parts.append(part)
        z[r] = sum(parts[::-1] if shuffled else parts)
    zc = np.clip(z, -fr.CLIP, fr.CLIP)
    return 1.0 / (1.0 + np.exp(-zc))


# --------------------------------------------------------------------------
# the raw ABI calls
# --------------------------------------------------------------------------
def plan_forward(rt, plan, dev, params, n_rows, register=False):
    """rfm_fm_plan_forward of the first n_rows rows of ``dev`` (a forward_rows_common.DeviceRows) into
    a NaN-filled buffer with guard elements behind it; ``register``: the log registered in slot 1 for
    the call (and unregistered after it)."""
    import torch
    import grad_forms_common as gf
    from relevance_factorizationmachine_amd import _lib
    if register:
        _lib.check(rt.lib.rfm_fm_plan_register_log(rt.ctx, plan.handle, 1, *dev.csr_ptrs(), n_rows))
    out = torch.full((n_rows + gf.GUARD,), float("nan"), dtype=torch.float64, device=rt.torch_device)
    _lib.check(rt.lib.rfm_fm_plan_forward(rt.ctx, plan.handle, *dev.csr_ptrs(), n_rows, *params.ptrs(), out.data_ptr()))
    rt.sync()
    if register:
        _lib.check(rt.lib.rfm_fm_plan_register_log(rt.ctx, plan.handle, 1, None, None, None, 0))
    got = out.cpu().numpy()
    assert np.isnan(got[n_rows:]).all(), "a score past the rows of the launch was written"
    return got[:n_rows]


def waves_rows(rows_per_wg):
    """Rows of the busiest wavefront of a workgroup of the sliced forward (16 wavefronts)."""
    return -(-rows_per_wg // 16)
