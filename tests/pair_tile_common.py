"""Shared by the pinning tests of the catalogue kernels (test_pair_tile_host.py,
test_gpu_pair_tile.py; csrc/rfm_pairs.hip): long-double oracles of the pair
logit and of the side sums with the magnitude each of them adds up, the tolerances derived from
those, a NumPy statement of the tile's sum that carries four mutations, a host model of the
ranking kernel's staging area, the case lists, and thin wrappers of the raw ABI calls.  Importing
this module touches neither the GPU nor the package under test.

The pair logit is z = ((c + LU[u]) + LI[i]) + sum_f A[u,f] B[i,f] and its magnitude
S_z = |c| + |LU[u]| + |LI[i]| + sum_f |A[u,f] B[i,f]|.  With u = 2^-53:

logit   |dz| <= (kpad + 8) u S_z.  A chain of kpad fused multiply-adds, in whatever order the
        chunks and the matrix core's k-slots take the factors, is off by at most kpad u of its
        absolute sum; the 8 covers the three adds in front of it.
score   |dp| <= p (1 - p) tol_z (1 + tol_z) + 8 u p, the form of forward_rows_common.tol_p: the
        logit's error through the sigmoid's slope, and 3 ulp of exp with the add and the divide.
A[r,f]  |dA| <= L_r u a_rf, a_rf = sum_j |x_j V[j,f]| over the row's L_r stored entries (as they
        are stored: no sorting, no merging): a sum of L_r rounded products.  The padding columns
        k .. kpad-1 are exactly +0.0, an empty row's A is +0.0 throughout.
L[r]    the side's L = lin + cross / 2, lin = sum_j x_j w_j, cross = sum_f (s_f^2 - q_f),
        s_f = A[r,f], q_f = sum_j x_j^2 V[j,f]^2.  With S_lin = sum_j |x_j w_j| and
        S_cross = sum_f (a_rf^2 + q_f):
          - lin, L_r rounded products summed: L_r u S_lin;
          - s_f is off by L_r u a_rf, so s_f^2 by 2 L_r u a_rf^2, and its own rounding adds
            u a_rf^2; q_f, a sum of L_r products of three roundings each: (L_r + 3) u q_f; the
            subtraction: u (a_rf^2 + q_f).  Per factor at most (2 L_r + 4) u (a_rf^2 + q_f);
          - a lane adds the factors f, f + 64, ...: ceil(kpad / 64) adds; the xor tree over the
            64 lanes: 6 more; each is off by at most u of the absolute sum: (ceil(kpad / 64) + 6)
            u S_cross;
          - the halving is exact; the last add: u (S_lin + S_cross / 2).
        |dL| <= (L_r + 1) u S_lin + (2 L_r + ceil(kpad / 64) + 12) u S_cross / 2.

All of them are derived, not measured.  The floor (test_pair_tile_host.py): the float64 statement
of each sum, in natural and in a shuffled order, stays below half of every tolerance on every case
-- with one exception that the derivation itself explains: A[r,f] of a ONE-entry row is one
rounded product, its tolerance u |x v| is that rounding's own bound, and so the floor there is the
whole tolerance, not half of it (every other row of the side matrix has six entries or more).

Inputs: A, B ~ N(0,1) kpad^(-1/4) (so that A.B has a standard deviation of 1 at every factor
count), LU, LI ~ N(0, 0.5^2), c = 0.37.  The host test asserts for every case list that every score
lies inside (1e-6, 1 - 1e-6), that at least 99 % of the adjacent positions of every user's oracle
order are SEPARATED, and that a dropped last factor moves at least 99 % of the logits by more than
tol_z.  Separated is taken more strictly than the sum of the two neighbours' tol_z: by more than
twice the largest tol_z of the user's row, because an item has to keep its distance from every
item in front of it, not only from its neighbour.

The list lengths of the ranking kernel: catalogues around every power of two from 512 to 4 096 and
depths around the same powers.  Two classes need a case of their own: the list length P = 256
needs min(depth, n_items) <= 256, hence n_items = 200 and the depths 200 and 256; a flush between
two passes at P = 4096 needs more than four passes of 1 024 items, hence n_items = 5 121.  A pass
is shorter than the list at P = 2 048 and 4 096, so there a `falling` row keeps appending until
its list is full (two and four passes) and appends nothing after that."""
import contextlib
import functools

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
C0 = 0.37
CLIP = 700.0
# the tile's shape as the host statement restates it; test_pair_tile_host.py holds both to
# rfm_pair_geometry
TILE, CHUNK = 64, 32
SENTINEL_BYTE = 0x5A
SENTINEL_I32 = np.frombuffer(bytes([SENTINEL_BYTE]) * 4, dtype=np.int32)[0]
SENTINEL_F64 = np.frombuffer(bytes([SENTINEL_BYTE]) * 8, dtype=np.float64)[0]  # about 1.7e130
GUARD = 64  # sentinel elements behind an output


def pad4(k):
    return (int(k) + 3) // 4 * 4


# --------------------------------------------------------------------------
# the pair oracle
# --------------------------------------------------------------------------
class Pairs:
    """Logit, magnitude, score and tolerances of every (selected user, item) pair (np.longdouble)."""

    def __init__(self, z, S_z, kpad):
        self.z, self.S_z, self.kpad = z, S_z, kpad
        with np.errstate(invalid="ignore", over="ignore"):
            self.zc = np.where(np.isnan(z), z, np.clip(z, -LD(CLIP), LD(CLIP)))
            self.p = 1 / (1 + np.exp(-self.zc))
        self.tol_z = LD(kpad + 8) * LD(U) * S_z
        self.tol_p = self.p * (1 - self.p) * self.tol_z * (1 + self.tol_z) + 8 * LD(U) * self.p

    def take(self, rows):
        out = Pairs.__new__(Pairs)
        out.kpad = self.kpad
        for name in ("z", "S_z", "zc", "p", "tol_z", "tol_p"):
            setattr(out, name, getattr(self, name)[rows])
        return out


def pair_oracle(A, LU, B, LI, c, user_ids=None):
    """``Pairs`` of the selected users (None: every user) against every item; a user id outside the
    table gives a row of NaN.  A, B are [n, k]: the padding adds nothing."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    n_users = A.shape[0]
    ids = np.arange(n_users) if user_ids is None else np.asarray(user_ids, dtype=np.int64)
    ok = (ids >= 0) & (ids < n_users)
    rows = np.where(ok, ids, 0)
    a, b = A.astype(LD)[rows], B.astype(LD)
    lu, li = np.asarray(LU).astype(LD)[rows], np.asarray(LI).astype(LD)
    with np.errstate(invalid="ignore", over="ignore"):
        z = ((LD(c) + lu)[:, None] + li[None, :]) + a @ b.T
        S = (abs(LD(c)) + np.abs(lu))[:, None] + np.abs(li)[None, :] + np.abs(a) @ np.abs(b).T
    z[~ok], S[~ok] = np.nan, np.nan
    return Pairs(z, S, pad4(A.shape[1]))


def pair_dense_ld(A, LU, B, LI, c):
    """The plain statement: one factor after the other, no matrix product."""
    a, b = np.asarray(A).astype(LD), np.asarray(B).astype(LD)
    z = (LD(c) + np.asarray(LU).astype(LD))[:, None] + np.asarray(LI).astype(LD)[None, :]
    for f in range(a.shape[1]):
        z = z + a[:, f, None] * b[None, :, f]
    return z


def pair_float64(A, LU, B, LI, c, order=None):
    """The float64 statement of the logit, the factors in ``order`` (None: as stored)."""
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    acc = np.zeros((A.shape[0], B.shape[0]))
    for f in (range(A.shape[1]) if order is None else order):
        acc += A[:, f, None] * B[None, :, f]
    return ((c + np.asarray(LU))[:, None] + np.asarray(LI)[None, :]) + acc


def sigmoid64(z):
    with np.errstate(over="ignore", invalid="ignore"):
        return 1.0 / (1.0 + np.exp(-np.clip(z, -CLIP, CLIP)))


def excess(got, want, tol):
    """|got - want| / tol per element; inf where finiteness disagrees, 0 where neither is finite or
    where the difference and the tolerance are both zero."""
    got = np.asarray(got, dtype=np.float64)
    want_finite = np.isfinite(want)
    with np.errstate(invalid="ignore", divide="ignore"):
        d = np.abs(got.astype(LD) - want)
        ratio = np.where(d == 0, LD(0), d / tol)
    ratio = np.where(want_finite & np.isfinite(got), ratio, np.inf)
    return np.where(~want_finite & ~np.isfinite(got), 0.0, ratio).astype(np.float64)


def assert_within(got, want, tol, what, bound=1.0):
    """Every element of ``got`` within ``bound * tol`` of ``want``; returns the largest ratio."""
    got = np.asarray(got, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ex = excess(got, want, tol)
    worst = float(ex.max()) if ex.size else 0.0
    print(f"{what}: largest |d| / tol {worst:.3g}")
    if not worst <= bound:
        at = np.unravel_index(int(np.argmax(ex)), ex.shape)
        raise AssertionError(f"{what}: {int((~(ex <= bound)).sum())} of {ex.size} elements outside {bound} * tol; "
                             f"worst at {at}: got {got[at]!r}, want {float(want[at])!r}, |d| / tol {ex[at]!r}")
    return worst


# --------------------------------------------------------------------------
# the order of a user's candidates
# --------------------------------------------------------------------------
def oracle_order(o, row, excluded=None):
    """The candidates of row ``row`` of the oracle (not NaN, not ``excluded``: a bool mask by item)
    under the total order (logit descending, then item index descending) ->
    ``(items, separated, need)``: position r is separated when its logit is more than ``need`` =
    twice the row's largest tol_z away from both neighbours."""
    z = o.z[row]
    cand = ~np.isnan(z)
    if excluded is not None:
        cand &= ~np.asarray(excluded)
    idx = np.flatnonzero(cand)
    order = idx[np.lexsort((-idx, -z[idx]))]
    need = 2 * (o.tol_z[row][cand].max() if idx.size else LD(0))
    wide = (z[order][:-1] - z[order][1:]) > need
    sep = np.ones(order.shape[0], dtype=bool)
    sep[1:] &= wide
    sep[:-1] &= wide
    return order, sep, need


def separated_share(o, excluded=None):
    """The smallest share, over the rows, of adjacent positions of the oracle order that are separated."""
    share = 1.0
    for r in range(o.z.shape[0]):
        order, _, need = oracle_order(o, r, None if excluded is None else excluded[r])
        if order.size > 1:
            share = min(share, float(np.mean((o.z[r][order][:-1] - o.z[r][order][1:]) > need)))
    return share


def oracle_lists(o, depth, users=None, excluded=None):
    """``(items int32 [n, depth] padded with -1, separated bool [n, depth], n_ranked int32 [n])`` of
    the selected rows of the oracle; ``excluded``: bool mask [rows of o, n_items]."""
    users = np.arange(o.z.shape[0]) if users is None else np.asarray(users)
    per = {}
    items = np.full((len(users), depth), -1, dtype=np.int32)
    sep = np.zeros((len(users), depth), dtype=bool)
    n_ranked = np.zeros(len(users), dtype=np.int32)
    for s, u in enumerate(users):
        u = int(u)
        if u not in per:
            per[u] = oracle_order(o, u, None if excluded is None else excluded[u])
        order, sp, _ = per[u]
        n = min(depth, order.shape[0])
        items[s, :n], sep[s, :n], n_ranked[s] = order[:n], sp[:n], order.shape[0]
        sep[s, n:] = True  # the padding is exact
    return items, sep, n_ranked


def oracle_rank(o, row, item, excluded=None):
    """``(rank, separated)`` of ``item`` for row ``row``: the number of candidates other than the item
    that are better than it (-1: its logit is NaN); separated as in ``oracle_order``."""
    z = o.z[row]
    if np.isnan(z[item]):
        return -1, True
    cand = ~np.isnan(z)
    if excluded is not None:
        cand &= ~np.asarray(excluded)
    cand[item] = False
    idx = np.flatnonzero(cand)
    if idx.size == 0:
        return 0, True
    better = (z[idx] > z[item]) | ((z[idx] == z[item]) & (idx > item))
    need = 2 * max(o.tol_z[row][idx].max(), o.tol_z[row][item])
    return int(better.sum()), bool(np.abs(z[idx] - z[item]).min() > need)


# --------------------------------------------------------------------------
# the side sums
# --------------------------------------------------------------------------
class Side:
    """A CSR side matrix as it is stored (repeated and unsorted columns stay as they are)."""

    def __init__(self, rows, n_cols):
        self.n_cols = n_cols
        self.indptr = np.concatenate([[0], np.cumsum([len(c) for c, _ in rows])]).astype(np.int64)
        self.indices = np.concatenate([np.asarray(c, dtype=np.int32) for c, _ in rows])
        self.data = np.concatenate([np.asarray(x, dtype=np.float64) for _, x in rows])
        self.n_rows = len(rows)


SIDE_COLS = 40
SIDE_ROW_NAMES = ("200 entries", "one entry", "empty", "a stored zero", "a column named twice",
                  "negative and non-binary", "first and last column", "random", "binary")
SIDE_FACTORS = (1, 3, 4, 5, 63, 64, 65, 127, 128, 129, 400)
SIDE_ROW_CUTS = (1, 3, 4, 5)


@functools.lru_cache(maxsize=None)
def side_matrix():
    rng = np.random.default_rng(2121)
    n = SIDE_COLS
    rows = [
        (rng.integers(0, n, size=200), rng.standard_normal(200)),
        ([17], [-1.75]),
        ([], []),
        ([3, 8, 11, 20, 21, 30, 33], [0.5, -1.25, 0.0, 2.0, 0.3, -0.7, 1.1]),
        ([5, 30, 2, 5, 19, 38, 7, 12, 26], [1.5, -0.4, 0.9, -2.2, 0.6, 1.0, -1.3, 0.25, 0.8]),
        ([1, 4, 9, 16, 25, 36, 22, 13], [-0.3, -1.7, -2.9, -0.01, -3.3, -0.6, -1.1, -0.45]),
        ([0, 39, 10, 20, 29, 31], [1.2, -0.8, 0.4, 2.1, -1.6, 0.7]),
        (rng.permutation(n)[:12], rng.standard_normal(12)),
        ([2, 6, 14, 23, 35, 39], [1.0] * 6),
    ]
    assert len(rows) == len(SIDE_ROW_NAMES)
    return Side(rows, n)


@functools.lru_cache(maxsize=None)
def side_parameters(n_factors):
    rng = np.random.default_rng(4000 + n_factors)
    w, V = rng.standard_normal(SIDE_COLS), 0.3 * rng.standard_normal((SIDE_COLS, n_factors))
    w.setflags(write=False)
    V.setflags(write=False)
    return w, V


class SideSums:
    pass


def side_oracle(X, w, V):
    """A [n_rows, kpad], L [n_rows] of the header in np.longdouble with their tolerances."""
    k = V.shape[1]
    kpad = pad4(k)
    o = SideSums()
    o.kpad, o.length = kpad, np.diff(X.indptr)
    o.A, o.mag_A = np.zeros((X.n_rows, kpad), dtype=LD), np.zeros((X.n_rows, kpad), dtype=LD)
    o.L, o.S_lin, o.S_cross = (np.zeros(X.n_rows, dtype=LD) for _ in range(3))
    Vl, wl = np.asarray(V).astype(LD), np.asarray(w).astype(LD)
    for r in range(X.n_rows):
        lo, hi = X.indptr[r], X.indptr[r + 1]
        cols, x = X.indices[lo:hi], X.data[lo:hi].astype(LD)
        vx = Vl[cols] * x[:, None]
        q = (vx * vx).sum(axis=0)
        o.A[r, :k], o.mag_A[r, :k] = vx.sum(axis=0), np.abs(vx).sum(axis=0)
        lin = wl[cols] * x
        o.S_lin[r] = np.abs(lin).sum()
        o.S_cross[r] = (o.mag_A[r, :k] ** 2 + q).sum()
        o.L[r] = lin.sum() + ((o.A[r, :k] ** 2 - q).sum()) / 2
    n = o.length.astype(LD)
    o.tol_A = n[:, None] * LD(U) * o.mag_A
    o.tol_L = (n + 1) * LD(U) * o.S_lin + (2 * n + (kpad + 63) // 64 + 12) * LD(U) * o.S_cross / 2
    return o


def side_float64(X, w, V, shuffle=None, q_takes_x_once=False):
    """The float64 statement of A and L, the entries of a row in stored order or, with a generator
    ``shuffle``, in a drawn one (the factors of L too).  ``q_takes_x_once``: a mutation, q_f adds
    x v^2 for x^2 v^2 -- the same number on a row of ones, which is what one-hot fixtures hold."""
    k = V.shape[1]
    A, L = np.zeros((X.n_rows, pad4(k))), np.zeros(X.n_rows)
    for r in range(X.n_rows):
        e = np.arange(X.indptr[r], X.indptr[r + 1])
        f = np.arange(k)
        if shuffle is not None:
            e, f = shuffle.permutation(e), shuffle.permutation(f)
        s, q, lin = np.zeros(k), np.zeros(k), 0.0
        for j in e:
            x, v = X.data[j], V[X.indices[j]]
            s += x * v
            q += (x if q_takes_x_once else x * x) * (v * v)
            lin += x * w[X.indices[j]]
        A[r, :k] = s
        cross = 0.0
        for t in (s * s - q)[f]:
            cross += t
        L[r] = lin + 0.5 * cross
    return A, L


# --------------------------------------------------------------------------
# inputs and case lists
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def operands(n_users, n_items, n_factors, seed=0):
    """``(A [n_users, k], LU, B [n_items, k], LI, c)``: computed once, shared, read-only."""
    rng = np.random.default_rng([n_users, n_items, n_factors, seed])
    scale = pad4(n_factors) ** -0.25
    A, B = scale * rng.standard_normal((n_users, n_factors)), scale * rng.standard_normal((n_items, n_factors))
    LU, LI = 0.5 * rng.standard_normal(n_users), 0.5 * rng.standard_normal(n_items)
    for a in (A, B, LU, LI):
        a.setflags(write=False)
    return A, LU, B, LI, C0


@functools.lru_cache(maxsize=None)
def case(n_users, n_items, n_factors, seed=0):
    """Operands and their oracle: computed once, shared, never modified."""
    ops = operands(n_users, n_items, n_factors, seed)
    return ops, pair_oracle(*ops)


# every tail quarter q = 1 .. 8 after 0, 1 and 3 full chunks, then the padded operands (kpad > k)
# and the ABI's upper bound
TILE_SHAPE = (65, 129)  # 2 x 3 tiles, the edge tiles one wide
KPAD_CLASSES = tuple(range(4, 33, 4)) + tuple(range(36, 65, 4)) + tuple(range(100, 129, 4))
TILE_FACTORS = KPAD_CLASSES + (1, 2, 3, 33, 34, 35, 125, 1024)
EDGE_SIZES = (1, 63, 64, 65, 128, 129)
EDGE_FACTORS = (5, 37)


def kpad_class(n_factors):
    """``(full chunks in front of the tail chunk, the tail chunk's factors per MFMA k-slot)``."""
    kpad = pad4(n_factors)
    chunks = (kpad + CHUNK - 1) // CHUNK
    return chunks - 1, (kpad - CHUNK * (chunks - 1)) // 4


# the walks: a 70-user table selected n_sel times
WALK_USERS = 70
WALK_SEL = (2112, 2049)
WALK_FACTORS = (5, 37)
# n_items -> (item tiles, tiles per split, splits, tiles of the last split) with 33 user tiles
WALK_ITEMS = {2049: (33, 2, 17, 1), 4160: (65, 3, 22, 2)}
WALK_K = (1, 9, 64)


@functools.lru_cache(maxsize=None)
def walk_selection(n_sel):
    rng = np.random.default_rng(n_sel)
    sel = np.concatenate([rng.permutation(WALK_USERS), rng.integers(0, WALK_USERS, size=n_sel - WALK_USERS)])
    sel.setflags(write=False)
    return sel.astype(np.int32)


WALK_EMPTY_SPLIT_USER, WALK_EMPTY_USER, WALK_NAN_ITEM = 3, 5, 100


def walk_exclusions(n_items, tiles_per_split, split=1):
    """Bool mask [70, n_items]: user 3 loses every item of split ``split``, user 5 every item, the
    others a tenth of the items at random."""
    rng = np.random.default_rng(n_items)
    M = rng.random((WALK_USERS, n_items)) < 0.1
    M[WALK_EMPTY_SPLIT_USER] = False
    M[WALK_EMPTY_SPLIT_USER, split * tiles_per_split * TILE: (split + 1) * tiles_per_split * TILE] = True
    M[WALK_EMPTY_USER] = True
    return M


def mask_csr(M):
    """``(indptr int64, items int32)`` of a bool mask: strictly ascending lists by row."""
    rows, cols = np.nonzero(M)
    return np.concatenate([[0], np.cumsum(M.sum(axis=1))]).astype(np.int64), cols.astype(np.int32)


def walk_targets(n_items, users):
    """Per selected user: item 0, the last item and three others, ascending -> (indptr, items)."""
    rng = np.random.default_rng(n_items + 1)
    mid = np.sort(rng.integers(1, n_items - 1, size=(len(users), 3)), axis=1)
    items = np.concatenate([np.zeros((len(users), 1), np.int64), mid, np.full((len(users), 1), n_items - 1)], axis=1)
    return np.arange(0, 5 * len(users) + 1, 5, dtype=np.int64), items.reshape(-1).astype(np.int32)


# the ranking kernel's list lengths (integer operands: rank_catalogue_common.expected_lists is exact)
ORDER_ITEMS = (200, 300, 512, 513, 1024, 1025, 2048, 2049, 3073, 4096, 5121)
ORDER_DEPTHS = (200, 256, 257, 512, 513, 1024, 1025, 2048, 2049)
ORDER_PATTERNS = ("rising", "falling", "three_values", "nan_items")
ORDER_LIST_LENGTHS = (256, 512, 1024, 2048, 4096)
ORDER_USERS, ORDER_FACTORS = 3, 4
ORDER_EXCLUDED_USER = 2  # with the exclusion lists: this user loses every item


def order_depths(n_items):
    """The depths of a catalogue: every listed depth it allows, n_items and n_items + 7."""
    return sorted({d for d in ORDER_DEPTHS if d <= n_items} | {n_items, n_items + 7})


def staging_walk(z, excluded, P, pass_len, threshold):
    """The ranking kernel's staging area on one row of logits, first page: per pass the number of
    appended candidates, the number of flushes between two passes, and the staged count of the last
    flush (0: none).  A host model for naming the situation a case is in; the lists themselves
    are checked against the definition."""
    z = np.asarray(z, dtype=np.float64)
    n = z.shape[0]
    cand = ~np.isnan(z)
    if excluded is not None:
        cand &= ~np.asarray(excluded)
    best = []  # (logit, item) sorted best first, at most P
    key = lambda e: (-e[0], -e[1])  # noqa: E731
    staged, appended, mid = [], [], 0
    for i0 in range(0, n, pass_len):
        if len(staged) > threshold:
            best = sorted(best + staged, key=key)[:P]
            staged, mid = [], mid + 1
        last = best[P - 1] if len(best) >= P else (-np.inf, -1)
        i = np.arange(i0, min(i0 + pass_len, n))
        i = i[cand[i] & ((z[i] > last[0]) | ((z[i] == last[0]) & (i > last[1])))]
        new = list(zip(z[i].tolist(), i.tolist()))
        assert len(staged) + len(new) <= P
        staged += new
        appended.append(len(new))
    return appended, mid, len(staged)


@functools.lru_cache(maxsize=None)
def order_case(pattern, n_items):
    """``(A, LU, B, LI, c, logit, excluded mask)`` of test_gpu_rank_catalogue._pattern_operands for 3
    users and 4 factors; the mask takes every item from ORDER_EXCLUDED_USER."""
    from test_gpu_rank_catalogue import _pattern_operands
    M = np.zeros((ORDER_USERS, n_items), dtype=bool)
    M[ORDER_EXCLUDED_USER] = True
    return _pattern_operands(pattern, ORDER_USERS, n_items, ORDER_FACTORS) + (M,)


def order_situations(n_items, depth, pattern):
    """The situations of the staging area that the case's rows are in, from the geometry query and
    the host model: "no flush between passes" (and a list to flush at the end), "a flush between
    passes", "a last flush of a count that is no power of two".  Asserts on the way that `rising`
    appends in every pass and `falling` in none once its list is full."""
    g = order_geometry(n_items, depth)
    logit, M = order_case(pattern, n_items)[5:]
    found = set()
    for u in range(ORDER_USERS):
        appended, mid, last = staging_walk(logit[u], M[u], g["P"], g["pass_len"], g["threshold"])
        if u != ORDER_EXCLUDED_USER and pattern == "rising":
            assert all(n > 0 for n in appended), (n_items, depth, appended)
        if u != ORDER_EXCLUDED_USER and pattern == "falling":
            full = g["P"] // g["pass_len"]  # passes that fill the list
            assert all(n > 0 for n in appended[:full]) and not any(appended[full:]), (n_items, depth, appended)
        if mid == 0 and last > 0:
            found.add("no flush between passes")
        if mid > 0:
            found.add("a flush between passes")
        if last > 0 and not is_power_of_two(last):
            found.add("a last flush of a count that is no power of two")
    return g, found


SITUATIONS = ("no flush between passes", "a flush between passes", "a last flush of a count that is no power of two")


def is_power_of_two(n):
    return n > 0 and n & (n - 1) == 0


# --------------------------------------------------------------------------
# the host statement of the tile, for mutations
# --------------------------------------------------------------------------
MUTATIONS = ("tail_drops_last_factor", "tail_runs_eight_quarters", "li_by_tile_local_item", "user_row_is_s")


def tile_statement(A, LU, B, LI, c, user_ids=None, mutation=None):
    """The tile's sum in float64 as the kernel orders it: the factors in chunks of 32, in a chunk of
    4 q factors step s of q gives MFMA k-slot j the factor j q + s; the item is i0 + il, the user row
    goes through ``user_ids`` (all inside the table here).  ``mutation``:

    - tail_drops_last_factor: the tail chunk leaves out the last factor;
    - tail_runs_eight_quarters: the tail chunk runs q = 8 over an LDS image whose upper part still
      holds the chunk before (nothing, when it is the first chunk);
    - li_by_tile_local_item: LI[il] for LI[i0 + il];
    - user_row_is_s: the operands of selected user s are row s (mod the table), not user_ids[s]."""
    assert mutation is None or mutation in MUTATIONS
    A, B = np.asarray(A, dtype=np.float64), np.asarray(B, dtype=np.float64)
    k, kpad = A.shape[1], pad4(A.shape[1])
    Ap, Bp = np.zeros((A.shape[0], kpad)), np.zeros((B.shape[0], kpad))
    Ap[:, :k], Bp[:, :k] = A, B
    n_items = B.shape[0]
    rows = np.arange(A.shape[0]) if user_ids is None else np.asarray(user_ids, dtype=np.int64)
    if mutation == "user_row_is_s":
        rows = np.arange(rows.shape[0]) % A.shape[0]
    acc = np.zeros((rows.shape[0], n_items))
    for k0 in range(0, kpad, CHUNK):
        width = min(CHUNK, kpad - k0)
        q = width // 4
        As, Bs = np.zeros((rows.shape[0], CHUNK)), np.zeros((n_items, CHUNK))
        As[:, :width], Bs[:, :width] = Ap[rows, k0:k0 + width], Bp[:, k0:k0 + width]
        tail = k0 + CHUNK >= kpad
        if tail and mutation == "tail_runs_eight_quarters":
            if k0 > 0:
                As[:, width:], Bs[:, width:] = Ap[rows, k0 - CHUNK + width:k0], Bp[:, k0 - CHUNK + width:k0]
            q = 8
        if tail and mutation == "tail_drops_last_factor":
            As[:, k - 1 - k0] = 0.0
        for s in range(q):
            for j in range(4):
                acc += As[:, j * q + s, None] * Bs[None, :, j * q + s]
    item = np.arange(n_items)
    li = np.asarray(LI)[item % TILE if mutation == "li_by_tile_local_item" else item]
    return ((c + np.asarray(LU)[rows])[:, None] + li[None, :]) + acc


# --------------------------------------------------------------------------
# the raw ABI calls
# --------------------------------------------------------------------------
GEOMETRY_NAMES = ("kpad", "chunks", "tail_quarter", "user_tiles", "item_tiles", "n_splits", "tiles_per_split",
                  "last_split_tiles")
ORDER_GEOMETRY_NAMES = ("P", "pass_len", "threshold", "pages")


def _library():
    from relevance_factorizationmachine_amd import _lib
    return _lib, _lib.load()


def geometry(n_sel, n_items, n_factors):
    """rfm_pair_geometry (host only) -> dict of GEOMETRY_NAMES."""
    _lib, lib = _library()
    out = np.full(8, -1, dtype=np.int64)
    _lib.check(lib.rfm_pair_geometry(int(n_sel), int(n_items), int(n_factors), out.ctypes.data_as(_int64_p())))
    return dict(zip(GEOMETRY_NAMES, (int(v) for v in out)))


def order_geometry(n_items, depth):
    """rfm_pair_order_geometry (host only) -> dict of ORDER_GEOMETRY_NAMES."""
    _lib, lib = _library()
    out = np.full(4, -1, dtype=np.int64)
    _lib.check(lib.rfm_pair_order_geometry(int(n_items), int(depth), out.ctypes.data_as(_int64_p())))
    return dict(zip(ORDER_GEOMETRY_NAMES, (int(v) for v in out)))


def _int64_p():
    import ctypes
    return ctypes.POINTER(ctypes.c_int64)


def topk_workspace(n_sel, n_items, k):
    import ctypes
    _lib, lib = _library()
    out = ctypes.c_int64(0)
    _lib.check(lib.rfm_pair_topk_workspace(int(n_sel), int(n_items), int(k), ctypes.byref(out)))
    return int(out.value)


def _filled(rt, shape, dtype):
    """A device tensor whose every byte is SENTINEL_BYTE."""
    import torch
    t = torch.empty(shape, dtype=dtype, device=rt.torch_device)
    t.view(-1).view(torch.uint8).fill_(SENTINEL_BYTE)
    return t


@contextlib.contextmanager
def sentinel_outputs(rt):
    """While it lasts, every buffer that a wrapper takes from ``rt.empty`` starts as sentinel bytes
    (the wrappers of the other test modules allocate their outputs there)."""
    rt.empty = lambda shape, dtype: _filled(rt, shape, dtype)
    try:
        yield
    finally:
        del rt.empty


def assert_written(*arrays):
    for a in arrays:
        sentinel = SENTINEL_I32 if a.dtype == np.int32 else SENTINEL_F64
        assert not (a == sentinel).any(), "an output element was not written"


def side_sums(rfm, X, w, V, n_rows=None):
    """rfm_fm_side_sums of the first ``n_rows`` rows of ``X`` (a Side) into sentinel-filled buffers of
    all its rows and a guard -> (A [X.n_rows, kpad], L [X.n_rows]) as the call left them."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    rt = rfm[3]
    k = V.shape[1]
    kpad = pad4(k)
    n_rows = X.n_rows if n_rows is None else n_rows
    d = [rt.upload(a) for a in (X.indptr, X.indices, X.data, *_own(w, V))]
    A = _filled(rt, (X.n_rows * kpad + GUARD,), torch.float64)
    L = _filled(rt, (X.n_rows + GUARD,), torch.float64)
    _lib.check(rt.lib.rfm_fm_side_sums(rt.ctx, d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), n_rows,
                                       d[3].data_ptr(), d[4].data_ptr(), X.n_cols, k, A.data_ptr(), L.data_ptr()))
    rt.sync()
    A, L = A.cpu().numpy(), L.cpu().numpy()
    assert (A[n_rows * kpad:] == SENTINEL_F64).all() and (L[n_rows:] == SENTINEL_F64).all(), \
        "an element past the rows of the launch was written"
    return A[:X.n_rows * kpad].reshape(X.n_rows, kpad), L[:X.n_rows]


def _own(*arrays):
    """Writable float64 copies (the shared cases are read-only; an upload wants its own array)."""
    return tuple(np.array(a, dtype=np.float64) for a in arrays)


def _padded(M):
    M = np.asarray(M, dtype=np.float64)
    out = np.zeros((M.shape[0], pad4(M.shape[1])))
    out[:, :M.shape[1]] = M
    return out


def scores(rfm, A, LU, B, LI, c, user_ids=None):
    """rfm_pair_scores into a sentinel-filled buffer with a guard behind it -> [n_sel, n_items]."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    rt = rfm[3]
    n_sel = A.shape[0] if user_ids is None else len(user_ids)
    n_items = B.shape[0]
    dA, dB, dLU, dLI = (rt.upload(a) for a in (_padded(A), _padded(B), *_own(LU, LI)))
    dc = rt.upload(np.array([c], dtype=np.float64))
    ids = None if user_ids is None else rt.upload(np.asarray(user_ids, dtype=np.int32))
    out = _filled(rt, (n_sel * n_items + GUARD,), torch.float64)
    _lib.check(rt.lib.rfm_pair_scores(rt.ctx, dA.data_ptr(), dLU.data_ptr(), A.shape[0],
                                      None if ids is None else ids.data_ptr(), n_sel, dB.data_ptr(), dLI.data_ptr(),
                                      n_items, A.shape[1], dc.data_ptr(), out.data_ptr()))
    rt.sync()
    got = out.cpu().numpy()
    assert (got[n_sel * n_items:] == SENTINEL_F64).all(), "an element past the output was written"
    got = got[:n_sel * n_items].reshape(n_sel, n_items)
    assert_written(got)
    return got


def topk(rfm, A, LU, B, LI, c, K, user_ids=None, excl=None):
    """rfm_pair_topk (test_gpu_recommend._abi_topk) into sentinel-filled outputs -> (items, scores)."""
    from test_gpu_recommend import _abi_topk
    with sentinel_outputs(rfm[3]):
        got = _abi_topk(rfm, *_own(A, LU, B, LI), c, K, user_ids=user_ids, excl=excl)
    assert_written(*got)
    return got


def ranks(rfm, A, LU, B, LI, c, tgt_indptr, tgt_items, user_ids=None, excl=None):
    """rfm_pair_ranks (test_gpu_rank_items._abi_ranks) -> (ranks, scores, candidates)."""
    from test_gpu_rank_items import _abi_ranks
    with sentinel_outputs(rfm[3]):
        got = _abi_ranks(rfm, *_own(A, LU, B, LI), c, tgt_indptr, tgt_items, user_ids=user_ids, excl=excl)
    assert_written(*got)
    return got


def order(rfm, A, LU, B, LI, c, depth, user_ids=None, excl=None):
    """rfm_pair_order (test_gpu_rank_catalogue._abi_order) -> (items, scores, n_ranked)."""
    from test_gpu_rank_catalogue import _abi_order
    with sentinel_outputs(rfm[3]):
        got = _abi_order(rfm, *_own(A, LU, B, LI), c, depth, user_ids=user_ids, excl=excl)
    assert_written(*got)
    return got
