"""Shared by the tests of MF fold-in (test_fold_in_host.py, test_gpu_fold_in.py): a long-double
statement of the fold-in semantics (the reference's per-example update,
src/mf.py:99-108 with :172-216, restricted to one side), an f64 restatement with the dot product
summed in the opposite order, case builders with a chosen geometry, the case list, and thin wrappers
of the raw ABI calls that keep every float array on the device between sentinels.  Importing this
module touches neither the GPU nor the library under test.

Comparison.  Folded rows are compared element by element against the largest magnitude of THEIR OWN
ROW in the oracle, biases against max(|want|, lr) (``mf_step_common.row_distance`` /
``bias_distance``); the fixed side, the weights and the sentinels around every array must keep
their bits.

Tolerance.  ``FOLD_TOL`` is not taken from a device result.  ``FOLD_FLOOR`` is the distance of the
f64 restatement with the reversed dot product from the long-double oracle on that scale, over every
case of the list (test_fold_in_host.py measures it on the CPU and holds the constant within 5%):
1.8e-15 (rows 9.1e-16, biases 1.8e-15); the recursion is contractive under ``reg``, so it stays flat
over the chains of 1 029 examples and three passes.  ``FOLD_TOL = min(64 * FOLD_FLOOR, 1e-11)`` =
1.2e-13; the margin covers the device's exp, division and FMA contraction.  The smallest error a
wrong read makes (a stale row, a skipped example) is lr * |err| * |q|, about 1e-2 of a row.
Largest distance an MI355X showed over the case list: 1.3e-15 (``GPU_MAX_SEEN``), below the CPU floor
and 90 times inside ``FOLD_TOL``."""
import functools
import zlib
from dataclasses import dataclass, field

import numpy as np

import fold_common
import mf_step_common as ms
from fold_common import FOLD_BLOCK, GRID_PER_CU, LD, N_FIXED, _chains, _sigmoid
from mf_step_common import B0, INIT_SEED, LR, REG, Guarded, PAD

FOLD_FLOOR = 1.8e-15                  # measured CPU floor to two digits (test_tolerance_floor holds it within 5%)
FOLD_TOL = min(64 * FOLD_FLOOR, 1e-11)
GPU_MAX_SEEN = 1.3e-15                # largest distance an MI355X showed (the grid case; 6.7e-16 over the listed cases)

DEPTH = 4                             # include/rfm_hip.h RFM_MF_FOLD_READ_AHEAD
LONG_CHAIN = 1029                     # the long chain of the small classes


def rows_per_workgroup(k):
    return FOLD_BLOCK // ms.shape_class(k)[0]


def grid_pass(k, n_cu):
    """New rows one pass of the capped grid covers."""
    return n_cu * GRID_PER_CU * rows_per_workgroup(k)


# --------------------------------------------------------------------------
# the semantics: one row, example by example (the form the mutations are made in)
# --------------------------------------------------------------------------
def fold_row(ids, ry, F, fb, x0, c0, n_passes, b=B0, lr=LR, reg=REG, dtype=LD, mutation=None):
    """One new row after ``n_passes`` passes over its examples: ``(x, c)`` in ``dtype``.
    ``mutation`` breaks the rule in one of four ways (test_fold_in_host.py): "stale" = the row
    update reads the row from before the previous example; "moves_fixed" = the fixed row is updated
    as the reference's Q is; "drops_last" = the last example is left out; "example_major" = every
    pass of an example before the next example."""
    ids = np.asarray(ids, dtype=np.int64)
    F, fb = np.array(F, dtype=dtype), np.array(fb, dtype=dtype)
    ry = np.asarray(ry).astype(dtype)
    x, c = np.array(x0, dtype=dtype), dtype(c0)
    b, lr, reg = dtype(b), dtype(lr), dtype(reg)
    n = len(ids) - (mutation == "drops_last" and len(ids) > 0)
    steps = [(p, e) for p in range(n_passes) for e in range(n)]
    if mutation == "example_major":
        steps = [(p, e) for e in range(n) for p in range(n_passes)]
    before = x.copy()
    for _, e in steps:
        j = ids[e]
        err = ry[e] - _sigmoid((x * F[j]).sum() + c + fb[j] + b, dtype)
        read = before if mutation == "stale" else x
        before = x
        x = x - lr * (-err * F[j] + reg * read)
        c = c - lr * (-err + reg * c)
        if mutation == "moves_fixed":
            F[j] = F[j] - lr * (-err * x + reg * F[j])
    return x, c


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------
@dataclass
class FoldCase(fold_common.FoldCaseBase):  # (N_FIXED fixed rows in every case but the anchor's)
    extra: dict = field(default_factory=dict)

    def fixed(self):
        """The fixed side ``(F [n_fixed, k], fb [n_fixed])``: the item side of the reference's init."""
        from oracle import cpu_ref
        _, Q, _, bi = cpu_ref.mf_init(INIT_SEED, 1, self.n_fixed, self.k)
        if self.clip:
            bi[0], bi[1] = 900.0, -900.0
        return Q, bi

    def start(self):
        """Initial ``(rows, bias)``: zeros, or a caller's values."""
        if not self.with_init:
            return np.zeros((self.n_new, self.k)), np.zeros(self.n_new)
        rng = np.random.default_rng(zlib.crc32(self.name.encode()) ^ 0x5EED)
        return rng.uniform(-1.0, 1.0, size=(self.n_new, self.k)), rng.normal(scale=0.1, size=self.n_new)


def fold_all(case, dtype=LD, reverse=False):
    """Every new row of a case after its passes, all rows at once step by step: ``(rows, bias)`` in
    ``dtype``.  ``reverse``: the dot product summed from the last factor to the first and the logit
    from its last term to the first (the f64 restatement the floor is measured with)."""
    F, fb = (np.asarray(a).astype(dtype) for a in case.fixed())
    X, C = (np.asarray(a).astype(dtype) for a in case.start())
    ry, ids, ptr, n = case.ry().astype(dtype), case.ids.astype(np.int64), case.row_ptr, case.lengths
    total = n * case.n_passes
    b, lr, reg = dtype(B0), dtype(LR), dtype(REG)
    for t in range(int(total.max()) if case.n_new else 0):
        act = np.flatnonzero(total > t)
        e = ptr[act] + t % n[act]
        j = ids[e]
        x, q, c = X[act], F[j], C[act]
        if reverse:
            z = b + fb[j] + c + ms._dot_reversed(x, q)
        else:
            z = (x * q).sum(axis=1) + c + fb[j] + b
        err = ry[e] - _sigmoid(z, dtype)
        X[act] = x - lr * (-err[:, None] * q + reg * x)
        C[act] = c - lr * (-err + reg * c)
    return X, C


def edge_lengths(depth=DEPTH):
    """Chain lengths around the read-ahead depth: its two rings are ``depth`` and ``2 * depth`` deep."""
    return [depth + 1, 0, 2 * depth, 1, depth - 1, 2 * depth + 1, depth, 2 * depth - 1]


SHAPE_KS = ms.SHAPE_KS                       # the lowest and highest k of the 19 classes, 300 and 400
LONG_KS = (1, 2, 3, 8)                       # the classes of four lanes per row: 16 rows to a wavefront
PASS_KS = (2, 33, 400, 1024)
COUNT_KS = (2, 16, 33, 400)
SPECIAL_KS = (7, 130)
GRID_K = 8


def shape_case(k):
    """a. rows whose chain lengths straddle the two rings, two passes; at four lanes per row one
    chain of 1 029 examples rides in the same wavefront."""
    lengths = edge_lengths() + ([LONG_CHAIN, 2] if k in LONG_KS else [])
    name = f"shape-k{k}"
    return FoldCase(name, k, _chains(name, lengths), 2)


def pass_case(k, n_passes):
    """b. the same chains under 0, 1, 2, 3 passes."""
    return FoldCase(f"passes{n_passes}-k{k}", k, _chains(f"passes-k{k}", edge_lengths() + [3, 2]), n_passes,
                    with_init=(n_passes == 0))


def count_cases(k):
    """c. 1, one short of a workgroup, a workgroup and one more rows."""
    gpb = rows_per_workgroup(k)
    out = []
    for n in sorted({1, gpb - 1, gpb, gpb + 1}):
        name = f"count{n}-k{k}"
        out.append(FoldCase(name, k, _chains(name, [(3 * r + 2) % 7 for r in range(n)]), 2))
    return out


def special_case(k, with_init):
    """d. a chain that names a fixed row twice in succession and again later; a fixed row (5) in
    every chain; logits driven past the clip on both sides (fixed rows 0, 1); a caller's init."""
    chains = [np.array([5, 7, 7, 3, 7, 9]), np.array([5, 0, 0, 4]), np.array([1, 5, 1]), np.array([5]),
              np.array([6, 5, 6, 6, 5, 5, 2, 6, 0, 1, 5])]
    return FoldCase(f"special{'-init' if with_init else ''}-k{k}", k, chains, 3, with_init=with_init, clip=True)


def grid_case(n_cu, k=GRID_K):
    """e. 37 rows more than one pass of the capped grid covers, chains of 0..2 examples.  The rows
    start from a caller's values of order 1: among 131 109 rows started at zero a few end where both
    examples' steps cancel to 1e-4 of either, and a comparison relative to the row's own magnitude
    then measures that cancellation (1.6e-12 in f64 at k = 2), not the arithmetic."""
    n = grid_pass(k, n_cu) + 37
    rng = np.random.default_rng(n)
    flat = rng.integers(0, N_FIXED, size=3 * n)
    chains = [flat[3 * r: 3 * r + (r * 7 + 1) % 3] for r in range(n)]
    return FoldCase(f"grid-k{k}", k, chains, 2, with_init=True)


@functools.lru_cache(maxsize=None)
def fold_cases():
    """Every case of a. to d. (e. depends on the device's CU count: ``grid_case``)."""
    out = [shape_case(k) for k in SHAPE_KS]
    out += [pass_case(k, p) for k in PASS_KS for p in (0, 1, 2, 3)]
    for k in COUNT_KS:
        out += count_cases(k)
    out += [special_case(k, init) for k in SPECIAL_KS for init in (False, True)]
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return {c.name: c for c in out}


oracle = fold_common.cached_oracle(fold_cases, fold_all)  # (rows, bias) in long double


def distance(got, want):
    """(largest row distance, largest bias distance) of ``got = (rows, bias)`` from the oracle."""
    rows = ms.row_distance(got[0], want[0]) if np.asarray(got[0]).size else np.zeros(1)
    bias = ms.bias_distance(got[1], want[1]) if np.asarray(got[1]).size else np.zeros(1)
    return float(rows.max()), float(bias.max())


def floor_of(case):
    return distance(fold_all(case, dtype=np.float64, reverse=True), oracle(case))


def assert_within(got, want, tol, what):
    """Folded ``(rows, bias)`` against the oracle, element by element.  Returns the largest distance."""
    worst = 0.0
    if np.asarray(got[0]).size:
        worst = max(ms.assert_rows_within(got[0], want[0], tol, f"{what} rows"),
                    ms.assert_bias_within(got[1], want[1], tol, f"{what} bias"))
    return worst


# --------------------------------------------------------------------------
# the raw ABI calls, every float array on the device between sentinels
# --------------------------------------------------------------------------
def geometry(n_new, k, rt=None):
    """rfm_mf_fold_geometry -> dict(lpr, vec, nc, rows, grid, depth); ``rt`` None: no context, the
    grid of a device of 256 CUs."""
    from relevance_factorizationmachine_amd import _lib
    out = np.zeros(6, dtype=np.int32)
    _lib.check(_lib.load().rfm_mf_fold_geometry(None if rt is None else rt.ctx, int(n_new), int(k), out.ctypes.data))
    return dict(zip(("lpr", "vec", "nc", "rows", "grid", "depth"), (int(v) for v in out)))


def run_fold(rt, case, start=None, n_passes=None):
    """rfm_mf_fold_in on a case from its start (or ``start``): ``(rows, bias)`` afterwards.  The
    fixed side, the weights and every sentinel are asserted to keep their bits."""
    from relevance_factorizationmachine_amd import _lib
    F, fb = case.fixed()
    x0, c0 = case.start() if start is None else start
    ry = case.ry()
    n_passes = case.n_passes if n_passes is None else n_passes
    k = case.k
    d_F, d_fb, d_ry = Guarded(rt, F, k), Guarded(rt, fb, PAD), Guarded(rt, ry, PAD)
    d_rows, d_bias = Guarded(rt, x0, k), Guarded(rt, c0, PAD)
    ints = fold_common.upload_ints(rt, case)
    _lib.check(rt.lib.rfm_mf_fold_in(
        rt.ctx, ints[0].data_ptr(), ints[1].data_ptr(), d_ry.ptr, ints[2].data_ptr(), case.n_new, d_F.ptr, d_fb.ptr,
        case.n_fixed, B0, k, LR, REG, n_passes, d_rows.ptr, d_bias.ptr))
    rt.sync()
    fold_common.assert_inputs_kept(case, ((d_F, F, "the fixed rows"), (d_fb, fb, "the fixed bias"), (d_ry, ry, "the weights")),
                                   ints)
    return d_rows.host().reshape(case.n_new, k), d_bias.host()
