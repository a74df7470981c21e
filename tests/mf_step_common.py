"""Shared by the tests of the exact MF batch step (test_mf_oracle_host.py, test_gpu_mf_step.py) and by
test_host_abi.py: a long-double statement of the sequential batch (src/mf.py:97-108, :172-216), a
Python restatement of the level schedule and of how the two launchers split it into launches, batch
builders with a chosen geometry, the case list, and thin wrappers of the raw ABI calls that keep
every device array between sentinels.  Importing this module touches neither the GPU nor the
library under test.

Comparison.  P and Q are compared element by element against the largest magnitude of THEIR OWN ROW
in the oracle, the biases against max(|want|, lr); rows of users / items outside the batch must keep
their initial bits.  One wrong row among thousands cannot hide in that.

Tolerance.  ``MF_TOL`` is not taken from a device result.  ``floor_of`` runs an f64 restatement of
the same loop with the dot product summed in the opposite order and measures its distance from the
long-double oracle on that scale, over every case of the list (test_mf_oracle_host.py does that on
the CPU).  Measured floor over the final case list: 8.9e-15 (rows 5.6e-15, biases 3.6e-15, scores
8.9e-15); it stays flat over the 1 029-level chains because ``reg`` makes the recursion
contractive.  ``MF_TOL = 64 * MF_FLOOR = 5.7e-13`` with ``MF_FLOOR`` the measured value to two
digits (the cap of 1e-11 is not reached): the margin covers the device's exp, division and FMA
contraction.  That is 1 700 times tighter than the norm-wise 1e-9 of the parity tests and about ten
orders below the smallest error a stale row read makes (lr * |err| * |q|, about 1e-2 of a row).
Largest distance an MI355X showed over the case list: 8.7e-15 (``GPU_MAX_SEEN``), a score of
rfm_mf_predict at k = 2; the largest of a parameter is 4.7e-15 (one wide level of 131 109 examples
at k = 2), so the device sits at the CPU floor, 65 times inside ``MF_TOL``.

Loss.  rfm_mf_predict_loss is held to the long-double loss of the long-double scores at ``LOSS_REL``.
A float64 score near 1 loses that under log(1 - pred + eps), in the reference as in the kernel (at
k = 1, 63 rows, numpy's float64 gives 4.653738930072743, an MI355X 4.653738930072744, long double
4.653738930455849), so ``predict_problem`` gives the rows with a logit in ``LOSS_BAND`` = (6, 50) a weight of
exactly 0 on that term; the float64 restatement then stays within 3.6e-15 of the long-double loss over every
scoring problem (``LOSS_FLOOR`` = 1e-13 is asserted on the CPU)."""
import functools
import zlib
from dataclasses import dataclass, field
from typing import Callable, Optional

import numpy as np

LD = np.longdouble

MF_FLOOR = 8.9e-15                    # measured CPU floor to two digits (test_tolerance_floor holds it within 5%)
MF_TOL = min(64 * MF_FLOOR, 1e-11)
GPU_MAX_SEEN = 8.7e-15                # largest distance an MI355X showed (a score at k = 2; parameters 4.7e-15)
LOSS_REL = 1e-12                      # the figure test_forward_loss_entry_point uses
LOSS_EPS = 1e-8                       # src/base.py:42
LOSS_BAND = (6.0, 50.0)               # logits at which float64 cannot hold LOSS_REL: see predict_problem
LOSS_FLOOR = LOSS_REL / 10            # what the float64 restatement of the loss must hold on the CPU

B0, LR, REG = 0.4, 0.02, 0.5          # global bias, learning rate, L2 of every case
INIT_SEED = 7

# ---- constants of the kernels' launch rules, each with the line it mirrors ----
LOGIT_CLIP = 700                      # src/base.py:65 (rfm_device_utils.hpp:10 kLogitClip)
MAX_FACTORS = 1024                    # include/rfm_hip.h:49 RFM_MAX_FACTORS
READ_AHEAD = 4                        # include/rfm_hip.h:51 RFM_MF_READ_AHEAD
NO_WRITER = 1 << 30                   # include/rfm_hip.h:53 RFM_MF_NO_WRITER
MF_BLOCK = 256                        # rfm_mf.hip kMfBlock
SEQ_BLOCK = 1024                      # rfm_mf.hip kSeqBlock
SEQ_BLOCK_CHUNKED = 512               # rfm_mf.hip seq_block(nc > 1)
SEQ_MAX_LEVELS = 1024                 # rfm_mf.hip kSeqMaxLevels
SEQ_MAX_RECS = 1024                   # rfm_mf.hip kSeqMaxRecs
GRID_PER_CU = 8                       # rfm_mf.hip capped_grid(..., 8, ...): mf_predict, launch_wide, the wide launch of rfm_mf_sgd_levels_ex
ASSUMED_CUS = 256                     # CUs the host-side geometry test assumes (an MI355X has 256)


def shape_class(k):
    """(lanes per row, factors per lane and chunk, chunks per lane): rfm_common.h:104-119."""
    assert 1 <= k <= MAX_FACTORS
    vec = 2 if k % 2 == 0 else 1
    units = -(-k // vec)
    lpr = 4
    while lpr < units and lpr < 64:
        lpr *= 2
    nc = 1
    while lpr * nc < units:
        nc *= 2
    if nc == 4 and lpr * 3 >= units:
        nc = 3
    return lpr, vec, nc


# lowest and highest factor count of each of the 19 classes
CLASS_RANGE = {
    (4, 1, 1): (1, 3), (4, 2, 1): (2, 8), (8, 1, 1): (5, 7), (8, 2, 1): (10, 16), (16, 1, 1): (9, 15),
    (16, 2, 1): (18, 32), (32, 1, 1): (17, 31), (32, 2, 1): (34, 64), (64, 1, 1): (33, 63),
    (64, 2, 1): (66, 128), (64, 1, 2): (65, 127), (64, 2, 2): (130, 256), (64, 1, 3): (129, 191),
    (64, 2, 3): (258, 384), (64, 1, 4): (193, 255), (64, 2, 4): (386, 512), (64, 1, 8): (257, 511),
    (64, 2, 8): (514, 1024), (64, 1, 16): (513, 1023),
}


def seq_cap(k, entry):
    """Largest level the sequential workgroup takes, the seq_cap each entry hands mf_walk_levels in
    rfm_mf.hip: rfm_mf_sgd_levels two passes of kSeqBlock threads, rfm_mf_sgd_levels_ex one pass of
    seq_block(nc) threads."""
    lpr, _, nc = shape_class(k)
    if entry == "levels":
        return 2 * (SEQ_BLOCK // lpr)
    assert entry == "levels_ex"
    return (SEQ_BLOCK_CHUNKED if nc > 1 else SEQ_BLOCK) // lpr


def grid_pass(k, n_cu):
    """Examples (or rows) one pass of a capped grid covers: n_cu * 8 workgroups of 256 / lpr."""
    return n_cu * GRID_PER_CU * (MF_BLOCK // shape_class(k)[0])


def launch_plan(level_ptr, k, entry):
    """The launches of one call: ``("wide", rec_lo, rec_hi)`` for a level above seq_cap,
    ``("seq", lev_lo, lev_hi)`` for a run of small levels.  Restates mf_walk_levels of rfm_mf.hip as
    the two entries call it (``levels``: no chunk limits, the run ends only at a wide level;
    ``levels_ex``: it also ends after kSeqMaxLevels levels and before the level that would take it
    past kSeqMaxRecs records)."""
    lp = [int(v) for v in level_ptr]
    n_levels, cap, plan, lev = len(lp) - 1, seq_cap(k, entry), [], 0
    while lev < n_levels:
        if lp[lev + 1] - lp[lev] > cap:
            plan.append(("wide", lp[lev], lp[lev + 1]))
            lev += 1
            continue
        end = lev
        while end < n_levels and lp[end + 1] - lp[end] <= cap:
            if entry == "levels_ex" and (end - lev >= SEQ_MAX_LEVELS or lp[end + 1] - lp[lev] > SEQ_MAX_RECS):
                break
            end += 1
        plan.append(("seq", lev, end))
        lev = end
    return plan


def levels_py(users, items):
    lu, li, lev = {}, {}, []
    for u, i in zip(users, items):
        l = max(lu.get(u, -1), li.get(i, -1)) + 1
        lu[u] = li[i] = l
        lev.append(l)
    return np.asarray(lev)


def gaps_py(users, lev):
    """Levels back to the previous writer of each example's user row (NO_WRITER if none)."""
    last, out = {}, []
    for u, l in zip(users, lev):
        out.append(NO_WRITER if u not in last else int(l) - last[u])
        last[u] = int(l)
    return np.asarray(out)


# --------------------------------------------------------------------------
# the oracle: long double, strictly sequential
# --------------------------------------------------------------------------
def _sigmoid_ld(z):
    return 1 / (1 + np.exp(-np.clip(z, -LD(LOGIT_CLIP), LD(LOGIT_CLIP))))


def is_disjoint(pairs):
    pairs = np.asarray(pairs)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


def mf_sgd_batch_ld(pairs, ry, P, Q, bu, bi, b, lr, reg, form=None):
    """One batch of src/mf.py:97-108 with :172-216 in np.longdouble; ``ry`` is label / propensity.
    Returns new (P, Q, b_u, b_i).  ``form``: "loop" walks the batch example by example; "disjoint"
    (every user and item once) updates all rows at once; None picks "disjoint" where it applies."""
    pairs = np.asarray(pairs, dtype=np.int64)
    P, Q, bu, bi = (np.array(a, dtype=LD) for a in (P, Q, bu, bi))
    ry = np.asarray(ry).astype(LD)
    b, lr, reg = LD(b), LD(lr), LD(reg)
    if form is None:
        form = "disjoint" if is_disjoint(pairs) else "loop"
    if form == "disjoint":
        assert is_disjoint(pairs)
        u, i = pairs[:, 0], pairs[:, 1]
        p, q = P[u], Q[i]
        err = ry - _sigmoid_ld((p * q).sum(axis=1) + bu[u] + bi[i] + b)
        p_new = p - lr * (-err[:, None] * q + reg * p)
        # the item row reads the user row this example has just updated (src/mf.py:193)
        Q[i] = q - lr * (-err[:, None] * p_new + reg * q)
        P[u] = p_new
        bu[u] = bu[u] - lr * (-err + reg * bu[u])
        bi[i] = bi[i] - lr * (-err + reg * bi[i])
        return P, Q, bu, bi
    assert form == "loop"
    for (u, i), r in zip(pairs, ry):
        err = r - _sigmoid_ld((P[u] * Q[i]).sum() + bu[u] + bi[i] + b)
        P[u] = P[u] - lr * (-err * Q[i] + reg * P[u])
        Q[i] = Q[i] - lr * (-err * P[u] + reg * Q[i])
        bu[u] = bu[u] - lr * (-err + reg * bu[u])
        bi[i] = bi[i] - lr * (-err + reg * bi[i])
    return P, Q, bu, bi


def mf_predict_ld(pairs, P, Q, bu, bi, b):
    """src/mf.py:136-170 in long double."""
    pairs = np.asarray(pairs, dtype=np.int64)
    u, i = pairs[:, 0], pairs[:, 1]
    dot = (np.asarray(P)[u].astype(LD) * np.asarray(Q)[i].astype(LD)).sum(axis=1)
    return _sigmoid_ld(dot + np.asarray(bu)[u].astype(LD) + np.asarray(bi)[i].astype(LD) + LD(b))


def ips_logloss_ld(y, pred_ld, pscore, eps=LOSS_EPS):
    """src/base.py:37-61 in long double."""
    r = np.asarray(y).astype(LD) / np.asarray(pscore).astype(LD)
    pred_ld, eps = np.asarray(pred_ld).astype(LD), LD(eps)
    return -(r * np.log(pred_ld + eps) + (1 - r) * np.log(1 - pred_ld + eps)).sum() / len(r)


# --------------------------------------------------------------------------
# the f64 restatement the tolerance floor is measured with
# --------------------------------------------------------------------------
def _sigmoid_f64(z):
    return 1.0 / (1.0 + np.exp(-np.clip(z, -700.0, 700.0)))


def _dot_reversed(p, q):
    """Sum of p*q over the last axis, strictly from the last factor to the first."""
    return np.cumsum((p * q)[..., ::-1], axis=-1)[..., -1]


def mf_sgd_batch_f64_reversed(pairs, ry, P, Q, bu, bi, b, lr, reg):
    pairs = np.asarray(pairs, dtype=np.int64)
    P, Q, bu, bi = (np.array(a, dtype=np.float64) for a in (P, Q, bu, bi))
    ry = np.asarray(ry, dtype=np.float64)
    if is_disjoint(pairs):
        u, i = pairs[:, 0], pairs[:, 1]
        p, q = P[u], Q[i]
        err = ry - _sigmoid_f64(b + bi[i] + bu[u] + _dot_reversed(p, q))
        p_new = p - lr * (-err[:, None] * q + reg * p)
        Q[i] = q - lr * (-err[:, None] * p_new + reg * q)
        P[u] = p_new
        bu[u] = bu[u] - lr * (-err + reg * bu[u])
        bi[i] = bi[i] - lr * (-err + reg * bi[i])
        return P, Q, bu, bi
    for (u, i), r in zip(pairs, ry):
        err = r - _sigmoid_f64(b + bi[i] + bu[u] + _dot_reversed(P[u], Q[i]))
        P[u] = P[u] - lr * (-err * Q[i] + reg * P[u])
        Q[i] = Q[i] - lr * (-err * P[u] + reg * Q[i])
        bu[u] = bu[u] - lr * (-err + reg * bu[u])
        bi[i] = bi[i] - lr * (-err + reg * bi[i])
    return P, Q, bu, bi


def mf_predict_f64_reversed(pairs, P, Q, bu, bi, b):
    pairs = np.asarray(pairs, dtype=np.int64)
    u, i = pairs[:, 0], pairs[:, 1]
    return _sigmoid_f64(b + bi[i] + bu[u] + _dot_reversed(P[u], Q[i]))


# --------------------------------------------------------------------------
# comparison
# --------------------------------------------------------------------------
def row_distance(got, want_ld):
    """|got - want| of every element over the largest |want| of its row (inf where got is NaN or a
    row of zeros is missed)."""
    got, want_ld = np.asarray(got, dtype=np.float64), np.asarray(want_ld)
    assert got.shape == want_ld.shape and got.ndim == 2, (got.shape, want_ld.shape)
    diff = np.abs(got.astype(LD) - want_ld)
    scale = np.abs(want_ld).max(axis=1, keepdims=True)
    with np.errstate(divide="ignore", invalid="ignore"):
        d = np.where(diff == 0, LD(0), diff / scale)
    return np.where(np.isnan(d), LD(np.inf), d)


def bias_distance(got, want_ld, lr=LR):
    got, want_ld = np.asarray(got, dtype=np.float64), np.asarray(want_ld)
    assert got.shape == want_ld.shape and got.ndim == 1, (got.shape, want_ld.shape)
    d = np.abs(got.astype(LD) - want_ld) / np.maximum(np.abs(want_ld), LD(lr))
    return np.where(np.isnan(d), LD(np.inf), d)


def score_distance(got, want_ld):
    got, want_ld = np.asarray(got, dtype=np.float64), np.asarray(want_ld)
    assert got.shape == want_ld.shape, (got.shape, want_ld.shape)
    d = np.abs(got.astype(LD) - want_ld) / np.maximum(want_ld, LD(1e-300))
    return np.where(np.isnan(d), LD(np.inf), d)


def _assert_small(d, tol, what, got, want_ld):
    bad = ~(d <= LD(tol))
    if bad.any():
        i = np.unravel_index(int(np.argmax(d)), d.shape)
        raise AssertionError(f"{what}: {int(bad.sum())} of {d.size} elements outside {tol}; worst at {i}: got "
                             f"{np.asarray(got)[i]!r}, want {float(np.asarray(want_ld)[i])!r}, distance {float(d[i]):.3e}")
    return float(d.max()) if d.size else 0.0


def assert_rows_within(got, want_ld, tol, what):
    return _assert_small(row_distance(got, want_ld), tol, what, got, want_ld)


def assert_bias_within(got, want_ld, tol, what, lr=LR):
    return _assert_small(bias_distance(got, want_ld, lr), tol, what, got, want_ld)


def assert_scores_within(got, want_ld, tol, what):
    return _assert_small(score_distance(got, want_ld), tol, what, got, want_ld)


def assert_params_within(got, want_ld, init, pairs, tol, what):
    """(P, Q, b_u, b_i) of a device against the oracle, element by element; rows and biases of users
    and items outside the batch against the initial bits.  Returns the largest distance."""
    pairs = np.asarray(pairs)
    worst = 0.0
    for idx, (name, col) in enumerate((("P", 0), ("Q", 1), ("b_u", 0), ("b_i", 1))):
        g, w, start = np.asarray(got[idx]), want_ld[idx], np.asarray(init[idx])
        worst = max(worst, (assert_rows_within if g.ndim == 2 else assert_bias_within)(g, w, tol, f"{what} {name}"))
        rest = np.setdiff1d(np.arange(len(start)), pairs[:, col])
        np.testing.assert_array_equal(g[rest], start[rest], err_msg=f"{what}: a row of {name} outside the batch changed")
    return worst


# --------------------------------------------------------------------------
# batch builders: (users, items) in batch order with the intended levels
# --------------------------------------------------------------------------
def from_levels(levels):
    """``levels[t]`` = the (user, item) pairs meant for level t; emitted level by level.  The
    intention is checked against ``levels_py``."""
    users = np.asarray([u for lv in levels for u, _ in lv], dtype=np.int64)
    items = np.asarray([i for lv in levels for _, i in lv], dtype=np.int64)
    want = [t for t, lv in enumerate(levels) for _ in lv]
    assert levels_py(users.tolist(), items.tolist()).tolist() == want, "the builder's levels are not the schedule's"
    return users, items


def disjoint(n):
    return np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64)


def chains(n_chains, n_levels, user_period, item_kind):
    """``n_chains`` parallel chains of ``n_levels`` levels.  Chain c at level t uses user
    ``base_c + t % period_c``, so its user row was last written exactly ``period_c`` levels back.
    ``item_kind``: "cached" / "uncached" = one item per chain (the two differ in the cache_cap the
    case schedules with); "fresh" = a new item at every level, on one user (period 1)."""
    periods = [user_period] * n_chains if np.isscalar(user_period) else list(user_period)
    assert len(periods) == n_chains and item_kind in ("cached", "uncached", "fresh")
    assert item_kind != "fresh" or set(periods) == {1}
    base = np.concatenate([[0], np.cumsum(periods)])
    levels = []
    for t in range(n_levels):
        levels.append([(int(base[c]) + t % periods[c], c * n_levels + t if item_kind == "fresh" else c)
                       for c in range(n_chains)])
    return from_levels(levels)


GAP_CYCLE = [u for p in range(1, 6) for u in 2 * [p * 10 + j for j in range(p)]]  # 30 users-in-order


def gap_chain(n_levels, phase):
    """ONE single-item chain whose users cycle through blocks of period 1, 2, 3, 4, 5 (each block:
    its p users twice), starting ``phase`` positions into the cycle of 30."""
    assert len(GAP_CYCLE) == 30
    ids = {u: n for n, u in enumerate(sorted(set(GAP_CYCLE)))}
    return from_levels([[(ids[GAP_CYCLE[(t + phase) % 30]], 0)] for t in range(n_levels)])


def grow_then_shrink(first, tail_chains, tail_levels):
    """Level sizes ``first``, ``2 * first``, then ``tail_chains`` per level: every item of level 0
    comes back in level 1 (under a new user) and the first ``tail_chains`` of them in every level of
    the tail."""
    assert tail_chains <= first
    levels = [[(a, a) for a in range(first)],
              [(a, first + a) for a in range(first)] + [(first + a, a) for a in range(first)]]
    for t in range(tail_levels):
        levels.append([(2 * first + 2 * a + t % 2, a) for a in range(tail_chains)])
    return from_levels(levels)


def repeats(n_items, times, n_users, n_once, once_users):
    """``n_items`` items ``times`` times each in levels of ``n_users`` examples (users 0..n_users-1
    in every level), with ``n_once`` items that occur once riding along on ``once_users`` more
    users, from level 0 on."""
    assert n_items % n_users == 0
    per_round = n_items // n_users
    levels = [[] for _ in range(times * per_round)]
    for r in range(times):
        for j in range(n_items):
            levels[r * per_round + j // n_users].append((j % n_users, j))
    for m in range(n_once):
        levels[m // once_users].append((n_users + m % once_users, n_items + m))
    return from_levels(levels)


def start_slots(n_wide, n_tail):
    """A wide level 0, then four chains that begin at levels 1, 2, 3, 4 -- the first four levels of
    the launch behind the wide one -- each on a user whose row the WIDE level wrote last (gap 1..4).
    Chain j's item is held at level j by new users until the chain begins."""
    nu = ni = 0
    levels = [[] for _ in range(4 + n_tail)]
    for j in range(4):
        w, a, item, other = nu, nu + 1, ni, ni + 1
        nu, ni = nu + 2, ni + 2
        levels[0] += [(a, item), (w, other)]
        for l in range(1, j + 1):
            levels[l].append((nu, item))
            nu += 1
        for l in range(j + 1, j + 1 + n_tail):
            levels[l].append((w, item))
    while len(levels[0]) < n_wide:
        levels[0].append((nu, ni))
        nu, ni = nu + 1, ni + 1
    return from_levels(levels)


def concat(*parts, skip0):
    """The parts one after the other in batch order, on ids of their own (from 1 on if ``skip0``)."""
    users, items, u0, i0 = [], [], int(skip0), int(skip0)
    for pu, pi in parts:
        users.append(np.asarray(pu) + u0)
        items.append(np.asarray(pi) + i0)
        u0, i0 = int(users[-1].max()) + 1, int(items[-1].max()) + 1
    return np.concatenate(users), np.concatenate(items)


# --------------------------------------------------------------------------
# the cases
# --------------------------------------------------------------------------
@dataclass
class Case:
    name: str
    k: int
    users: np.ndarray
    items: np.ndarray
    want_plan: dict                      # entry -> the launches the case is named for
    cache_cap: Optional[int] = None      # None: rfm_mf_cache_capacity(k)
    check: Optional[Callable] = None     # (case, ex, level_ptr, cache_items): the state it is named for
    n_cu: int = ASSUMED_CUS
    extra: dict = field(default_factory=dict)

    @property
    def pairs(self):
        return np.stack([self.users, self.items], axis=1)

    @property
    def n_users(self):
        return int(self.users.max()) + 2  # (one row behind the last user stays outside the batch)

    @property
    def n_items(self):
        return int(self.items.max()) + 2

    def ry(self):
        """(label, propensity) of the batch, drawn as the parity tests draw them."""
        rng = np.random.default_rng(zlib.crc32(self.name.encode()))
        n = len(self.users)
        return (rng.random(n) < 0.5).astype(np.float64), rng.uniform(0.1, 1.0, size=n) ** 0.5

    def init(self):
        from oracle import cpu_ref
        return cpu_ref.mf_init(INIT_SEED, self.n_users, self.n_items, self.k)


def _has0(case):
    return bool((case.users == 0).any() and (case.items == 0).any())


def _chk_cached(n):
    def check(case, ex, lptr, cache):
        assert len(cache) == n, (len(cache), n)
        assert (ex["cslot"][np.isin(ex["i"], cache)] >= 0).all()
    return check


def _chk_ring(kind, n_chains):
    def check(case, ex, lptr, cache):
        finite = set(ex["gap"][ex["gap"] != NO_WRITER].tolist())
        cap = capacity(case.k) if case.cache_cap is None else case.cache_cap
        if kind == "fresh":
            assert finite == {1} and (ex["cslot"] == -1).all() and len(cache) == 0
        else:
            # both sides of the read-ahead boundary: written 4 levels back, and 5
            assert finite >= {1, 2, 3, 4, 5, 6} and {READ_AHEAD, READ_AHEAD + 1} <= finite
            assert len(cache) == min(n_chains, cap)
            want = {-2} if cap == 0 else ({0, -2} if cap < n_chains else {0})
            assert {min(int(c), 0) for c in ex["cslot"]} == want, want
        assert (np.diff(lptr) == n_chains).all()  # every level holds one example of every chain
        assert _has0(case) == case.extra["row0"]
    return check


def _chk_start_slots(case, ex, lptr, cache):
    wide_users = set(ex["u"][: lptr[1]].tolist())
    for j in range(READ_AHEAD):  # launch level j = level j + 1
        recs = ex[lptr[j + 1]: lptr[j + 2]]
        hit = recs[recs["gap"] == j + 1]
        assert len(hit) == 1 and int(hit["u"][0]) in wide_users and hit["cslot"][0] >= 0, (j, recs)


def _chk_cut(levels_before):
    """The launch that begins at ``levels_before`` reads rows written 1..4 levels before the cut, and
    cached items cross it."""
    def check(case, ex, lptr, cache):
        lev = np.repeat(np.arange(len(lptr) - 1), np.diff(lptr))
        assert len(cache) >= 1 and (ex["cslot"] != -2).all() and (ex["cslot"] >= 0).any()
        plan = case.want_plan["levels_ex"]
        assert set(levels_before) <= {lo for _, lo, _ in plan[1:]} and all(kind == "seq" for kind, _, _ in plan)
        for cut in levels_before:
            head = (lev >= cut) & (lev < cut + READ_AHEAD) & (ex["gap"] != NO_WRITER)
            back = cut - (lev[head] - ex["gap"][head])  # how far before the cut the writer lies
            assert {1, 2, 3, 4} <= set(back.tolist()), (cut, sorted(set(back.tolist())))
        for _, cut, _ in plan[1:]:  # cached items cross every cut
            assert set(ex["i"][lev < cut].tolist()) & set(ex["i"][lev >= cut].tolist()) & set(cache.tolist())
    return check


def _chk_grow(case, ex, lptr, cache):
    plan = case.want_plan["levels_ex"]
    assert [p[0] for p in plan] == ["seq", "wide", "seq"]
    lev = np.repeat(np.arange(len(lptr) - 1), np.diff(lptr))
    touched = [set(ex["i"][lev == 0].tolist()), set(ex["i"][lev == 1].tolist()), set(ex["i"][lev >= 2].tolist())]
    assert touched[0] & touched[1] & touched[2] & set(cache.tolist()), "no cached item is touched in all three launches"
    assert np.diff(lptr)[1] > np.diff(lptr)[0]  # the levels grow before they shrink


def _chk_beyond_cache(case, ex, lptr, cache):
    cap = capacity(case.k)
    assert cap == {3: 819, 400: 10}[case.k], cap  # 32 KiB of rows of k + 2 doubles
    assert len(cache) == cap, (len(cache), cap)
    slots = ex["cslot"]
    assert (slots >= 0).any() and (slots == -2).any() and (slots == -1).sum() == 10
    assert all(kind == "seq" for kind, _, _ in case.want_plan["levels_ex"])  # the cache is the sequential kernel's


def _seq_by_records(n_levels, per_level):
    """Launches of ``n_levels`` levels of ``per_level`` examples each, all small."""
    step = min(SEQ_MAX_LEVELS, SEQ_MAX_RECS // per_level)
    return [("seq", lo, min(lo + step, n_levels)) for lo in range(0, n_levels, step)]


def capacity(k):
    from relevance_factorizationmachine_amd.runtime import mf_cache_capacity
    return mf_cache_capacity(k)


SHAPE_KS = sorted({k for lo_hi in CLASS_RANGE.values() for k in lo_hi} | {300, 400})
RING_KS = (16, 128, 200, 300, 400, 513)   # chunks per lane 1, 1, 2, 3, 4 and 16 (no ring)
LIMIT_KS = (16, 300)
GRID_KS = (128, 2)
FIT_KS = (513, 1023, 1024)


def shape_case(k):
    """a. seq_cap + 3 disjoint pairs (one wide level under both entry points) in front of 3 chains
    of 24 levels, user periods 1, 4, 5, cached items; user 0 and item 0 absent."""
    n_wide = max(seq_cap(k, "levels"), seq_cap(k, "levels_ex")) + 3
    users, items = concat(disjoint(n_wide), chains(3, 24, [1, 4, 5], "cached"), skip0=True)
    plan = [("wide", 0, n_wide + 3), ("seq", 1, 24)]

    def check(case, ex, lptr, cache):
        _chk_cached(3)(case, ex, lptr, cache)
        assert not _has0(case) and capacity(k) >= 3
        assert {1, 4, 5} <= set(ex["gap"].tolist())
    return Case(f"shape-k{k}", k, users, items, {"levels": plan, "levels_ex": plan}, check=check)


def ring_cases(k):
    """b. the read-ahead ring."""
    cap_ex = seq_cap(k, "levels_ex")
    out = []
    six = [1, 2, 3, 4, 5, 6]
    for kind, row0 in (("cached", False), ("uncached", True), ("fresh", False)):
        periods = six if kind != "fresh" else 1
        users, items = concat(chains(6, 40, periods, kind), skip0=not row0)
        out.append(Case(f"ring-{kind}-k{k}", k, users, items, {"levels_ex": [("seq", 0, 40)]},
                        cache_cap=0 if kind == "uncached" else None, check=_chk_ring(kind, 6), extra={"row0": row0}))
    users, items = concat(chains(cap_ex, 40, [six[c % 6] for c in range(cap_ex)], "cached"), skip0=False)
    out.append(Case(f"ring-full-k{k}", k, users, items, {"levels_ex": _seq_by_records(40, cap_ex)},
                    check=_chk_ring("cached", cap_ex), extra={"row0": True}))
    n_wide = cap_ex + 3
    users, items = concat(start_slots(n_wide, 8), skip0=True)
    out.append(Case(f"ring-start-k{k}", k, users, items, {"levels_ex": [("wide", 0, n_wide), ("seq", 1, 12)]},
                    check=_chk_start_slots))
    return out


def limit_cases(k):
    """c. the launch limits."""
    out = []
    # 1024 % 30 == 4: phase 12 puts the second half of the period-4 block at levels 1024..1027
    for n in (1024, 1029):
        users, items = concat(gap_chain(n, 12), skip0=True)
        plan = [("seq", 0, 1024)] + ([("seq", 1024, n)] if n > 1024 else [])
        out.append(Case(f"limit-levels{n}-k{k}", k, users, items, {"levels_ex": plan},
                        check=_chk_cut([1024] if n > 1024 else [])))
    users, items = concat(chains(5, 300, [1, 2, 3, 4, 5], "cached"), skip0=True)
    out.append(Case(f"limit-recs1020-k{k}", k, users, items, {"levels_ex": [("seq", 0, 204), ("seq", 204, 300)]},
                    check=_chk_cut([204])))
    four = chains(4, 256, [1, 2, 3, 5], "cached")
    users, items = concat(four, skip0=True)
    out.append(Case(f"limit-recs1024-k{k}", k, users, items, {"levels_ex": [("seq", 0, 256)]}, check=_chk_cut([])))
    users, items = concat(four, disjoint(1), skip0=True)
    out.append(Case(f"limit-recs1025-k{k}", k, users, items, {"levels_ex": [("seq", 0, 255), ("seq", 255, 256)]},
                    check=_chk_cut([])))
    return out


def cache_cases():
    """c. seq -> wide -> seq at k = 300, and repeated items beyond the cache."""
    users, items = concat(grow_then_shrink(5, 3, 20), skip0=True)
    grow = Case("limit-grow-k300", 300, users, items,
                {"levels_ex": [("seq", 0, 1), ("wide", 5, 15), ("seq", 2, 22)]}, check=_chk_grow)
    # 1 500 items twice in 12 levels of 250 (+2 riders: 252 <= 256), 1 008 records to a launch
    users, items = concat(repeats(1500, 2, 250, 10, 2), skip0=True)
    many = Case("limit-cache-k3", 3, users, items, {"levels_ex": [("seq", 0, 4), ("seq", 4, 8), ("seq", 8, 12)]},
                check=_chk_beyond_cache)
    users, items = concat(repeats(20, 3, 5, 10, 3), skip0=True)
    few = Case("limit-cache-k400", 400, users, items, {"levels_ex": [("seq", 0, 12)]}, check=_chk_beyond_cache)
    return [grow, many, few]


def grid_case(k, n_cu):
    """d. one wide level of more examples than one pass of the capped grid covers."""
    n = grid_pass(k, n_cu) + 37
    users, items = concat(disjoint(n), skip0=True)

    def check(case, ex, lptr, cache):
        assert len(ex) > grid_pass(k, n_cu) and len(lptr) == 2
    return Case(f"grid-k{k}", k, users, items, {"levels_ex": [("wide", 0, n)]}, check=check, n_cu=n_cu)


@functools.lru_cache(maxsize=None)
def step_cases():
    """Every case of a., b. and c. (d. depends on the device's CU count: ``grid_case``)."""
    out = [shape_case(k) for k in SHAPE_KS]
    for k in RING_KS:
        out += ring_cases(k)
    for k in LIMIT_KS:
        out += limit_cases(k)
    out += cache_cases()
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return {c.name: c for c in out}


def reach(case, entry="levels_ex"):
    """The schedule of a case from the library's host scheduler, with the assertions that the case
    reaches the state it is named for: levels of ``levels_py``, the named launches, its own check.
    Returns ``(ex, level_ptr, cache_items)``."""
    from relevance_factorizationmachine_amd.runtime import mf_schedule_ex
    y, p = case.ry()
    cap = capacity(case.k) if case.cache_cap is None else case.cache_cap
    ex, lptr, cache = mf_schedule_ex(case.users, case.items, y, p, case.n_users, case.n_items, cap)
    lev = levels_py(case.users.tolist(), case.items.tolist())
    order = np.argsort(lev, kind="stable")
    np.testing.assert_array_equal(lptr, np.concatenate([[0], np.cumsum(np.bincount(lev))]))
    np.testing.assert_array_equal(ex["u"], case.users[order])
    np.testing.assert_array_equal(ex["i"], case.items[order])
    np.testing.assert_array_equal(ex["ry"], (y / p)[order])
    np.testing.assert_array_equal(ex["gap"], gaps_py(case.users.tolist(), lev)[order])
    assert launch_plan(lptr, case.k, entry) == case.want_plan[entry], (case.name, entry, launch_plan(lptr, case.k, entry))
    if case.check is not None:
        case.check(case, ex, lptr, cache)
    return ex, lptr, cache


@functools.lru_cache(maxsize=None)
def _oracle_by_name(name):
    case = step_cases()[name]
    return oracle_of(case)


def oracle_of(case):
    y, p = case.ry()
    return mf_sgd_batch_ld(case.pairs, y / p, *case.init(), B0, LR, REG)


def oracle(case):
    """(P, Q, b_u, b_i) after the batch, in long double; computed once per case."""
    return _oracle_by_name(case.name) if case.name in step_cases() else oracle_of(case)


def floor_of(case):
    """Distance of the f64 restatement (dot product summed backwards) from the oracle."""
    y, p = case.ry()
    got = mf_sgd_batch_f64_reversed(case.pairs, y / p, *case.init(), B0, LR, REG)
    want = oracle(case)
    rows = max(float(row_distance(got[0], want[0]).max()), float(row_distance(got[1], want[1]).max()))
    bias = max(float(bias_distance(got[2], want[2]).max()), float(bias_distance(got[3], want[3]).max()))
    return rows, bias


# --------------------------------------------------------------------------
# scoring cases (d.)
# --------------------------------------------------------------------------
def predict_problem(k, n_rows, with_ids):
    """``n_rows`` (user, item) pairs of a log of n_rows + 11 rows, read through ``row_ids`` (a
    permutation's head) or directly; the first two scored rows have their logit clipped at +700
    and -700 through the user's bias."""
    rng = np.random.default_rng(1000 * k + n_rows + int(with_ids))
    from oracle import cpu_ref
    nu, ni, n_log = 37, 23, n_rows + 11
    P, Q, bu, bi = cpu_ref.mf_init(INIT_SEED, nu, ni, k)
    users = rng.integers(2, nu, size=n_log)
    items = rng.integers(0, ni, size=n_log)
    ids = rng.permutation(n_log)[:n_rows].astype(np.int32) if with_ids else None
    sel = ids if with_ids else np.arange(n_rows)
    users[sel[0]] = 0
    bu[0] = 900.0
    if n_rows > 1:
        users[sel[1]] = 1
        bu[1] = -900.0
    y = (rng.random(n_log) < 0.5).astype(np.float64)
    p = rng.uniform(0.1, 1.0, size=n_log) ** 0.5
    # mf_init draws logits with a spread of 32 / sqrt(k).  A score is a float64, so near 1 it carries
    # an absolute rounding error of 1.1e-16, which log(1 - pred + eps) divides by exp(-z) + eps, in
    # the reference's own float64 as much as in the kernel.  With the term's weight |1 - y / p| up to
    # 2.2, that is 2.4e-16 * exp(z) of a loss of order 1: within LOSS_FLOOR = 1e-13 up to z = 6.  From
    # z = 37 the float64 score is exactly 1 and drops exp(-z) beside eps = 1e-8, which is below 1e-13
    # of the term from z = 49.  No float64 evaluation holds LOSS_REL against a long-double loss in
    # between, so the rows of LOSS_BAND = (6, 50) get label 1 at propensity 1, where the term's weight
    # is exactly 0.  Their scores are compared like every other, and a score near 0 has a relative
    # error only.
    z = (P[users] * Q[items]).sum(axis=1) + bu[users] + bi[items] + B0
    band = (z > LOSS_BAND[0]) & (z < LOSS_BAND[1])
    y[band], p[band] = 1.0, 1.0
    return {"k": k, "users": users, "items": items, "ids": ids, "sel": sel, "y": y, "p": p,
            "params": (P, Q, bu, bi), "n_rows": n_rows}


def predict_sizes(k, n_cu):
    gpb = MF_BLOCK // shape_class(k)[0]
    sizes = [1, gpb - 1, gpb + 1]
    if k in GRID_KS:
        sizes.append(grid_pass(k, n_cu) + 37)
    return sizes


def predict_floor(prob):
    pairs = np.stack([prob["users"], prob["items"]], axis=1)[prob["sel"]]
    want = mf_predict_ld(pairs, *prob["params"], B0)
    return float(score_distance(mf_predict_f64_reversed(pairs, *prob["params"], B0), want).max())


def predict_loss_floor(prob):
    """Relative distance of src/base.py:37-61 in float64, on the float64 scores with the dot product
    summed backwards, from the long-double loss of the long-double scores."""
    sel = prob["sel"]
    pairs = np.stack([prob["users"], prob["items"]], axis=1)[sel]
    want = float(ips_logloss_ld(prob["y"][sel], mf_predict_ld(pairs, *prob["params"], B0), prob["p"][sel]))
    pred = mf_predict_f64_reversed(pairs, *prob["params"], B0)
    r = prob["y"][sel] / prob["p"][sel]
    got = -np.sum(r * np.log(pred + LOSS_EPS) + (1.0 - r) * np.log(1.0 - pred + LOSS_EPS)) / len(r)
    return abs(got - want) / abs(want)


# --------------------------------------------------------------------------
# the raw ABI calls, every device array between sentinels
# --------------------------------------------------------------------------
SENTINEL_BITS = np.uint64(0x7FF8_5EA7_1E55_C0DE)  # a quiet NaN with a payload of its own
PAD = 8                                            # sentinel elements around a vector


class Guarded:
    """A float64 array on the device with ``pad`` sentinel elements before and after; ``ptr`` is the
    interior.  ``host()`` returns the interior and asserts the sentinels kept their bits."""

    def __init__(self, rt, values, pad):
        values = np.ascontiguousarray(values, dtype=np.float64)
        self.shape, self.size, self.pad = values.shape, values.size, pad
        flat = np.empty(self.size + 2 * pad, dtype=np.float64)
        flat.view(np.uint64)[:] = SENTINEL_BITS
        flat[pad: pad + self.size] = values.ravel()
        self.dev = rt.upload(flat)

    @classmethod
    def blank(cls, rt, n, pad=PAD):
        """``n`` elements that are sentinels themselves (an output buffer)."""
        values = np.empty(n, dtype=np.float64)
        values.view(np.uint64)[:] = SENTINEL_BITS
        return cls(rt, values, pad)

    @property
    def ptr(self):
        return self.dev.data_ptr() + 8 * self.pad

    def host(self, written=None):
        flat = self.dev.cpu().numpy()
        bits = flat.view(np.uint64)
        assert (bits[: self.pad] == SENTINEL_BITS).all(), "the sentinel in front of an array was written"
        assert (bits[self.pad + self.size:] == SENTINEL_BITS).all(), "the sentinel behind an array was written"
        if written is not None:
            assert (bits[self.pad + written: self.pad + self.size] == SENTINEL_BITS).all(), "an element past n_rows was written"
        return flat[self.pad: self.pad + self.size].reshape(self.shape).copy()


class DeviceParams:
    """P, Q (one sentinel ROW before and after), b_u, b_i (8 sentinel elements) on the device."""

    def __init__(self, rt, P, Q, bu, bi):
        self.rt = rt
        k = P.shape[1]
        self.arrays = [Guarded(rt, P, k), Guarded(rt, Q, k), Guarded(rt, bu, PAD), Guarded(rt, bi, PAD)]

    def ptrs(self):
        return tuple(a.ptr for a in self.arrays)

    def host(self):
        self.rt.sync()
        return tuple(a.host() for a in self.arrays)


def run_levels_ex(rt, case, sched, init):
    """rfm_mf_sgd_levels_ex on the schedule of ``reach``: (P, Q, b_u, b_i) afterwards."""
    from relevance_factorizationmachine_amd import _lib
    ex, lptr, cache = sched
    params = DeviceParams(rt, *init)
    d_ex = rt.upload(np.ascontiguousarray(ex).view(np.uint8))
    d_lptr = rt.upload(lptr)
    d_cache = rt.upload(cache) if len(cache) else None
    _lib.check(rt.lib.rfm_mf_sgd_levels_ex(
        rt.ctx, d_ex.data_ptr(), lptr.ctypes.data, d_lptr.data_ptr(), len(lptr) - 1,
        d_cache.data_ptr() if len(cache) else None, len(cache), *params.ptrs(), B0, case.k, LR, REG))
    return params.host()


def _as_log(case):
    """The batch as rows of a log in a shuffled order: (users, items, y, p of the log, pos_rows)."""
    y, p = case.ry()
    n = len(case.users)
    pos_rows = np.random.default_rng(n).permutation(n).astype(np.int32)
    users, items, ly, lp = (np.empty(n, dtype=t) for t in (np.int32, np.int32, np.float64, np.float64))
    users[pos_rows], items[pos_rows], ly[pos_rows], lp[pos_rows] = case.users, case.items, y, p
    return users, items, ly, lp, pos_rows


def run_levels(rt, case, init):
    """rfm_mf_schedule + rfm_mf_sgd_levels on the same batch."""
    from relevance_factorizationmachine_amd import _lib
    from relevance_factorizationmachine_amd.runtime import mf_schedule
    order, lptr = mf_schedule(case.users, case.items, case.n_users, case.n_items)
    assert launch_plan(lptr, case.k, "levels") == case.want_plan["levels"], launch_plan(lptr, case.k, "levels")
    users, items, y, p, pos_rows = _as_log(case)
    params = DeviceParams(rt, *init)
    dev = [rt.upload(a) for a in (users, items, y, p, pos_rows, order, lptr)]
    _lib.check(rt.lib.rfm_mf_sgd_levels(
        rt.ctx, *(d.data_ptr() for d in dev[:6]), lptr.ctypes.data, dev[6].data_ptr(), len(lptr) - 1,
        *params.ptrs(), B0, case.k, LR, REG))
    return params.host()


def run_hogwild(rt, case, init):
    from relevance_factorizationmachine_amd import _lib
    users, items, y, p, pos_rows = _as_log(case)
    params = DeviceParams(rt, *init)
    dev = [rt.upload(a) for a in (users, items, y, p, pos_rows)]
    _lib.check(rt.lib.rfm_mf_sgd_hogwild(rt.ctx, *(d.data_ptr() for d in dev), len(pos_rows), *params.ptrs(),
                                         B0, case.k, LR, REG))
    return params.host()


def run_predict(rt, prob, loss, want_pred=True):
    """rfm_mf_predict (``loss`` False) or rfm_mf_predict_loss: ``(scores or None, loss or None)``.
    The score buffer has 8 more elements than rows; they and the sentinels must stay as they were."""
    from relevance_factorizationmachine_amd import _lib
    params = DeviceParams(rt, *prob["params"])
    n = prob["n_rows"]
    du, di = rt.upload(prob["users"].astype(np.int32)), rt.upload(prob["items"].astype(np.int32))
    d_ids = rt.upload(prob["ids"]) if prob["ids"] is not None else None
    ids_ptr = d_ids.data_ptr() if d_ids is not None else None
    out = Guarded.blank(rt, n + 8) if want_pred else None
    if not loss:
        _lib.check(rt.lib.rfm_mf_predict(rt.ctx, du.data_ptr(), di.data_ptr(), ids_ptr, n, *params.ptrs(), B0,
                                         prob["k"], out.ptr))
        d_loss = None
    else:
        dy, dp = rt.upload(prob["y"]), rt.upload(prob["p"])
        d_loss = Guarded.blank(rt, 1)
        _lib.check(rt.lib.rfm_mf_predict_loss(rt.ctx, du.data_ptr(), di.data_ptr(), dy.data_ptr(), dp.data_ptr(),
                                              ids_ptr, n, *params.ptrs(), B0, prob["k"], LOSS_EPS,
                                              out.ptr if want_pred else None, d_loss.ptr))
    after = params.host()  # (synchronises; the parameters are inputs here and must not change)
    for a, b in zip(after, prob["params"]):
        np.testing.assert_array_equal(a, b)
    return (out.host(written=n)[:n] if want_pred else None), (float(d_loss.host()[0]) if loss else None)
