"""Shared by the tests of row addressing in wide tables (test_wide_tables_host.py,
test_gpu_wide_tables.py): tables of more than 2^32 bytes (T32b) or more than 2^31 elements (T31e),
where a row offset that is not formed in 64 bits wraps.  Importing this module touches neither the
GPU nor the package under test.

The method.  A case is a pair of problems: a COMPACT one of m ids, as the other common modules build
them, and its WIDE twin, whose ids are the compact ones under a strictly increasing map (`IdMap`)
into 0 .. n-1, n just past a threshold row T -- the first row whose offset no longer fits 32 bits of
bytes (T32b) or 31 bits of elements (T31e).  The map is strictly increasing, so every order relation
a plan or a schedule can depend on is the compact problem's.  The wide live ids are 0, the low ids,
T - 1, T, T + 1 of every threshold of the table and n - 1.  A wide table lives on the device only:
NaN everywhere (`torch.full`), the live rows put in from the compact host arrays.  Both problems
run through the same entry point of the C ABI and three things are asserted:

(a) outputs and the live rows of every written table equal the compact run (bit for bit where the
    project claims a fixed summation order, else within the bound the call's own module uses
    against its long-double oracle on the compact problem);
(b) the census: the non-NaN elements of a wide table after the call are live rows x width (a write
    through a wrapped offset lands on a guard row and changes the count, a read through one
    returns NaN or another live row's contents and fails (a));
(c) the sizes the case means: the table's bytes or elements past the threshold, and the byte or
    element offsets of the live ids on either side of it.

`MAPS` lists the id map of every GPU case by name; the GPU module takes its maps from here and the
host test holds every one of them to a NumPy model of a gather and a scatter whose offsets wrap
(`VirtualTable`): a wrapped variant must fail (a) or (b) on each of them."""
import numpy as np

T32B, T31E = "T32b", "T31e"
MARGIN = 5          # rows from the (largest) threshold row to the end of a table: T .. T + 4 = n - 1
MASK_T32B = (1 << 29) - 1   # element offsets of doubles that fit 32 bits of bytes
MASK_T31E = (1 << 31) - 1   # element offsets that fit a non-negative int
MASKS = {T32B: MASK_T32B, T31E: MASK_T31E}


def threshold_row(kind, width):
    """The first row of a table of `width` doubles per row whose element offset row * width does not
    fit: 2^29 elements = 2^32 bytes (T32b), 2^31 elements (T31e)."""
    limit = {T32B: 1 << 29, T31E: 1 << 31}[kind]
    return -(-limit // width)


class IdMap:
    """The strictly increasing map of the compact ids 0 .. m-1 into the wide ids 0 .. n-1 of a table
    of `width` doubles per row that crosses the thresholds `kinds`: the last compact ids go to
    T - 1, T, T + 1 of every threshold and to n - 1, the others stay what they are."""

    def __init__(self, m, width, kinds=(T32B,)):
        self.m, self.width, self.kinds = int(m), int(width), tuple(kinds)
        self.T = {kind: threshold_row(kind, width) for kind in self.kinds}
        self.n = max(self.T.values()) + MARGIN
        high = sorted({t + d for t in self.T.values() for d in (-1, 0, 1)} | {self.n - 1})
        low = self.m - len(high)
        assert low >= 3 and low < min(high), (m, high)   # id 0 and a few low ids
        self.wide = np.concatenate([np.arange(low), high]).astype(np.int64)
        assert len(self.wide) == self.m and np.all(np.diff(self.wide) > 0)

    def __call__(self, ids):
        return self.wide[np.asarray(ids, dtype=np.int64)]

    def compact(self, wide_id):
        """The compact id that maps to `wide_id` (which must be live)."""
        at = int(np.searchsorted(self.wide, wide_id))
        assert self.wide[at] == wide_id
        return at

    @property
    def top(self):
        """The largest threshold row of the table."""
        return max(self.T.values())

    def assert_sizes(self, numel=None):
        """(c): the table is past every threshold it names, and the live ids T - 1 and T lie on
        either side of each."""
        numel = self.n * self.width if numel is None else numel
        for kind, t in self.T.items():
            if kind == T32B:
                assert numel * 8 > 2 ** 32
                assert (t - 1) * self.width * 8 < 2 ** 32 <= t * self.width * 8
            else:
                assert numel > 2 ** 31
                assert (t - 1) * self.width < 2 ** 31 <= t * self.width
            assert {t - 1, t, t + 1} <= set(self.wide.tolist())
        assert self.wide[0] == 0 and self.wide[-1] == self.n - 1

    def describe(self, what):
        size = self.n * self.width * 8 / 2 ** 30
        return (f"{what}: {self.n} rows x {self.width} doubles = {size:.3f} GiB; crossed "
                + ", ".join(f"{kind} at row {t}" for kind, t in self.T.items()))


# --------------------------------------------------------------------------
# the id maps of the GPU cases: name -> (compact ids, doubles per row, thresholds)
# --------------------------------------------------------------------------
FM_COLS = 40        # columns of a compact FM log
FM_COLS_BOUNDED = 96  # ... of one whose rows hold at most 16 entries (the 8-lane forward)
MF_PREDICT_USERS, MF_PREDICT_ITEMS = 37, 23   # mf_step_common.predict_problem
PAIR_ITEMS = 131    # items of a compact pair problem: two tiles of 64 and three items
PAIR_USERS = 5

MAPS = {}


def _register(name, m, width, kinds=(T32B,)):
    assert name not in MAPS
    MAPS[name] = (m, width, tuple(kinds))


for _k in (32, 128, 1024):
    _register(f"fm-V-k{_k}", FM_COLS, _k)
_register("fm-V-k32-bounded", FM_COLS_BOUNDED, 32)
_register("fm-V-k1024-T31e", FM_COLS, 1024, (T32B, T31E))
_register("mf-P-predict-k128", MF_PREDICT_USERS, 128)
_register("mf-Q-predict-k128", MF_PREDICT_ITEMS, 128)
_register("mf-P-predict-k1024-T31e", MF_PREDICT_USERS, 1024, (T32B, T31E))
_register("mf-fold-F-k128", 23, 128)                # the fixed rows of fold_in_common.shape_case
_register("pair-B-kpad1024", PAIR_ITEMS, 1024)
_register("pair-B-kpad1024-T31e", PAIR_ITEMS, 1024, (T32B, T31E))
_register("pair-A-kpad1024", 9, 1024)             # the rows of pair_tile_common.side_matrix
_register("fm-V-k128-bounded", FM_COLS_BOUNDED, 128)   # the generic forward on padded row blocks
_register("fm-fold-new-k1024", 8, 1024)           # the new rows of fm_fold_common.pass_case(1024, 2)
_register("mf-fold-new-k128", 8, 128)             # the new rows of fold_in_common.shape_case(128)
_register("audience-A-kpad1024", PAIR_ITEMS, 1024)    # by-item entries: the candidates are the users
_register("audience-B-kpad1024", 9, 1024)         # ... and the queries the items

# rfm_pair_scores into a wide OUTPUT: its rows are the selected users, n_items doubles each
WIDE_OUT_ITEMS = (1 << 22) + 5
WIDE_OUT_SEL = -(-(1 << 29) // WIDE_OUT_ITEMS) + MARGIN


def id_map(name):
    """The map of a GPU case."""
    return IdMap(*MAPS[name])


# MF step cases take their user / item counts from mf_step_common's builders; the maps are made
# per case with `step_map`, and the host test walks the same builders
# name -> (factor count, thresholds): 128 the largest factor count of the single-chunk 64-lane class,
# 1024 the largest of all (8 chunks per lane)
MF_STEP_CASES = {"shape-k128": (128, (T32B,)), "shape-k1024-T31e": (1024, (T32B, T31E))}


def mf_step_case(name):
    """shape_case: one wide level in front of a sequential run of 24 levels on cached items."""
    import mf_step_common as ms
    return ms.shape_case(MF_STEP_CASES[name][0])


def step_map(name, n_ids):
    k, kinds = MF_STEP_CASES[name]
    return IdMap(n_ids, k, kinds)


# --------------------------------------------------------------------------
# the NumPy model: a virtual wide table and accesses whose offsets wrap
# --------------------------------------------------------------------------
def element_offsets(ids, width, wrap=None):
    """Element offsets [len(ids), width] of the rows `ids`, formed correctly (wrap None) or reduced
    to what fits 32 bits of bytes (T32B) / 31 bits of elements (T31E)."""
    e = np.asarray(ids, dtype=np.int64)[:, None] * width + np.arange(width, dtype=np.int64)[None, :]
    return e if wrap is None else e & MASKS[wrap]


class VirtualTable:
    """A table of n rows x width doubles held as its live rows alone: NaN everywhere else."""

    def __init__(self, n, width, live, rows):
        self.n, self.width = int(n), int(width)
        rows = np.asarray(rows, dtype=np.float64).reshape(len(live), width)
        self.cells = {}
        for i, row in zip(np.asarray(live, dtype=np.int64).tolist(), rows):
            for c in range(width):
                self.cells[i * width + c] = float(row[c])

    def gather(self, ids, wrap=None):
        e = element_offsets(ids, self.width, wrap)
        assert e.min() >= 0 and e.max() < self.n * self.width   # (a mask only lowers an offset)
        return np.array([[self.cells.get(int(x), np.nan) for x in row] for row in e])

    def scatter(self, ids, rows, wrap=None):
        e = element_offsets(ids, self.width, wrap)
        assert e.min() >= 0 and e.max() < self.n * self.width
        for row_e, row in zip(e, np.asarray(rows, dtype=np.float64).reshape(len(ids), self.width)):
            for x, v in zip(row_e.tolist(), row.tolist()):
                self.cells[x] = v

    def census(self):
        return sum(1 for v in self.cells.values() if not np.isnan(v))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool((a.view(np.int64) == b.view(np.int64)).all())


def model_verdicts(live, n, width, wrap, seed=0):
    """What the harness sees of a kernel whose row offsets wrap as `wrap` (None: a correct kernel) on
    a table with the live ids `live`: ``(gather_ok, scatter_ok)``.  The gather is (a) of a read-only
    call -- the rows gathered from the wide table against the compact rows.  The scatter is (a) and
    (b) of a writing call -- new rows written to every live id, then the live rows read back
    correctly against the compact result, and the census against live rows x width."""
    rng = np.random.default_rng(seed)
    live = np.asarray(live, dtype=np.int64)
    rows = rng.standard_normal((len(live), width))
    table = VirtualTable(n, width, live, rows)
    gather_ok = same_bits(table.gather(live, wrap), rows)
    new = rng.standard_normal((len(live), width))
    table.scatter(live, new, wrap)
    scatter_ok = same_bits(table.gather(live), new) and table.census() == len(live) * width
    return gather_ok, scatter_ok


# --------------------------------------------------------------------------
# wide tables on the device (torch is imported by the callers' process only when these run)
# --------------------------------------------------------------------------
GIB = 1 << 30
SLAB = 1 << 27      # elements of a census slab: 1 GiB of doubles, 128 MiB of flags


def assert_room(rt, n_bytes):
    """`n_bytes` of tables and 2 GiB beside them are free on the device."""
    import torch
    free, _ = torch.cuda.mem_get_info(rt.torch_device)
    assert free > n_bytes + 2 * GIB, f"{free / GIB:.1f} GiB free, the case needs {n_bytes / GIB:.1f} GiB"


LIVE_TABLES = []    # every wide tensor a case made: freed by `free_tables` whoever still refers to it


def nan_table(rt, shape):
    """A float64 device tensor of NaN, registered for `free_tables`."""
    import torch
    t = torch.full(shape, float("nan"), dtype=torch.float64, device=rt.torch_device)
    LIVE_TABLES.append(t)
    return t


def free_tables():
    """Give the memory of every registered table back to the device.  The storage is emptied in
    place, so a table that a failed case's traceback still refers to is freed as well and cannot
    leave the next case short of room."""
    import gc
    import torch
    while LIVE_TABLES:
        t = LIVE_TABLES.pop()
        t.untyped_storage().resize_(0)
        del t
    gc.collect()
    torch.cuda.empty_cache()


def wide_table(rt, n, width, live, rows):
    """A float64 table [n, width] (width None: [n]) on the device: NaN, with `rows` at the ids `live`."""
    import torch
    shape = (int(n),) if width is None else (int(n), int(width))
    t = nan_table(rt, shape)
    idx = torch.from_numpy(np.asarray(live, dtype=np.int64)).to(rt.torch_device)
    t.index_put_((idx,), rt.upload(np.ascontiguousarray(rows, dtype=np.float64).reshape((len(live),) + shape[1:])))
    return t


def census(t):
    """Non-NaN elements of a device tensor, counted on the device in slabs."""
    flat = t.reshape(-1)
    total = 0
    for at in range(0, flat.numel(), SLAB):
        s = flat[at: at + SLAB]
        total += int(s.numel()) - int(s.isnan().sum())
    return total


def count_nonzero(t):
    """Elements of a device tensor that are not zero (NaN counts), in slabs."""
    flat = t.reshape(-1)
    return sum(int((flat[at: at + SLAB] != 0).sum()) for at in range(0, flat.numel(), SLAB))


def live_rows(t, live):
    """The rows `live` of a device table, on the host."""
    import torch
    idx = torch.from_numpy(np.asarray(live, dtype=np.int64)).to(t.device)
    return t.index_select(0, idx).cpu().numpy()


def assert_census(t, n_live_rows, what):
    width = 1 if t.dim() == 1 else int(t.shape[1])
    got = census(t)
    assert got == n_live_rows * width, \
        f"{what}: {got} elements of the wide table are not NaN, {n_live_rows} live rows x {width} = {n_live_rows * width}"


def assert_same_bits(got, want, what):
    got, want = np.ascontiguousarray(got, dtype=np.float64), np.ascontiguousarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.int64) != want.view(np.int64)
    if bad.any():
        i = tuple(int(v) for v in np.argwhere(bad)[0])
        raise AssertionError(f"{what}: {int(bad.sum())} of {got.size} elements differ from the compact run; "
                             f"first at {i}: wide {got[i]!r}, compact {want[i]!r}")


class WideFmParams:
    """w0, w [n] and V [n, k] of a wide FM problem on the device; the interface of
    grad_forms_common.Params as far as the ABI wrappers use it (`ptrs`, `n`, `k`)."""

    def __init__(self, rt, imap, w0, w, V):
        self.rt, self.imap = rt, imap
        self.n, self.k = imap.n, V.shape[1]
        assert imap.width == self.k and len(w) == imap.m
        self.w0 = rt.upload(w0, dtype=np.float64)
        self.w = wide_table(rt, self.n, None, imap.wide, w)
        self.V = wide_table(rt, self.n, self.k, imap.wide, V)

    def ptrs(self):
        return self.w0.data_ptr(), self.w.data_ptr(), self.V.data_ptr()

    def live(self):
        """(w0, w, V) at the live ids, on the host: the shapes of the compact problem."""
        self.rt.sync()
        return self.w0.cpu().numpy(), live_rows(self.w, self.imap.wide), live_rows(self.V, self.imap.wide)

    host = live   # (what adagrad_common.adagrad_step returns of its params)

    def assert_census(self, what):
        self.rt.sync()
        assert_census(self.V, self.imap.m, f"{what} V")
        assert_census(self.w, self.imap.m, f"{what} w")

    def assert_sizes(self):
        self.imap.assert_sizes(self.V.numel())


def widen_log(log, imap):
    """The log with its columns under the map: a CSR of imap.n columns (the entries keep their order)."""
    from scipy.sparse import csr_matrix
    X = log["features"]
    assert X.shape[1] == imap.m
    W = csr_matrix((X.data.copy(), imap(X.indices).astype(np.int32), X.indptr.copy()), shape=(X.shape[0], imap.n))
    return {"features": W, "labels": log["labels"], "pscores": log["pscores"]}


def move_column(log, theta, src, dst):
    """The compact problem with the columns `src` and `dst` exchanged (log and parameters alike)."""
    from scipy.sparse import csr_matrix
    X = log["features"]
    perm = np.arange(X.shape[1])
    perm[[src, dst]] = perm[[dst, src]]
    Y = csr_matrix(X[:, perm])
    Y.sort_indices()
    w0, w, V = theta
    return {"features": Y, "labels": log["labels"], "pscores": log["pscores"]}, (w0, w[perm].copy(), V[perm].copy())
