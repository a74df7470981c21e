"""Shared by the tests that hold a call on a USED FM plan to the same call on a fresh plan
(test_plan_history_host.py, test_gpu_plan_history.py): the logs, the id generators, the sequences of
calls as data, a long-double gradient oracle that works on the entries of the CSR, and thin wrappers
of the raw ABI calls that grad_forms_common / forward_rows_common do not have.  Importing this module
touches neither the GPU nor the package under test.

A call is ``Call(entry, shape, ids, opt)``:

entry   step (rfm_fm_step under SGD), step_ada (the same after set_optimizer(ADAGRAD)), grad
        (rfm_fm_grad), rows (rfm_fm_grad_rows; opt "ranges": with owner ranges), rows_empty
        (rfm_fm_grad_rows of no rows), train (rfm_fm_train, TRAIN_ITERS iterations, no loss outputs),
        train_loss (the same with both losses; opt "big": a validation log of the many-rows shape; "ride":
        RIDE_ITERS iterations, enough for the form whose loss rows ride in the next step's forward), plan_forward
        (rfm_fm_plan_forward of the log registered in slot 1).
shape   the rows of the batch, by name (``host_sizes``; the GPU tests resolve the names from
        rfm_fm_forward_geometry): one, group (a workgroup of the one-row shape + 1), below (the largest
        one-row launch), min, min+1, trip2 (= the plan's max_batch: workgroup 0 makes a second trip);
        on the plan of k = 400, whose max_batch is 3 000: one, group, mid, max.  "zero" / "val" for
        the two entries that take no batch.
ids     how the batch's row ids relate to those of the batch before: fresh (a new draw), same,
        disjoint, overlap (half of them from the batch before); "-" where there are none.

Which calls advance the plan's step counter (read in enqueue_step and rfm_fm_grad_rows): every call
that reaches enqueue_step does, once per launch of the three kernels -- step, step_ada, grad and rows
by one, train and train_loss by one per iteration.  rows_empty (enqueue_grad_rows skips enqueue_step
for an empty shard; only touch_seq moves) and plan_forward do not.  `increments` states that; the
host test holds the chunked sequences to both parities with it."""
import functools
from collections import namedtuple

import numpy as np
from scipy.sparse import csr_matrix

import forward_rows_common as fr
import grad_forms_common as gf

LD = np.longdouble
EDGES = (0, 1, 8, 9, 15, 16)   # row lengths of test_gpu_forward_lanes8.EDGES
N_FREQ, N_SPARSE = 24, 2000
N_COLS = N_FREQ + N_SPARSE
EXTRA_ROWS = 300               # rows of a log beyond the plan's max_batch
VAL_SMALL, VAL_BIG = 150, 1300
TRAIN_ITERS = 3
RIDE_ITERS = 5                 # iterations of a call whose loss rows ride in the next step's forward (at least 4)
STEP_LR = 2.0 ** -13           # (batch-SUM gradients of up to 65 000 rows)
MAX_CALLS = 64

ENTRIES = ("step", "step_ada", "grad", "rows", "rows_empty", "train", "train_loss", "plan_forward")
UNSHAPED = {"rows_empty": "zero", "plan_forward": "val"}
ADVANCE = {"step": 1, "step_ada": 1, "grad": 1, "rows": 1, "rows_empty": 0, "train": TRAIN_ITERS,
           "train_loss": TRAIN_ITERS, "plan_forward": 0}
IDS_KINDS = ("fresh", "same", "disjoint", "overlap")
SHAPE_CLASS = {"one": "small", "group": "small", "below": "small", "mid": "small",
               "min": "large", "min+1": "large", "trip2": "large", "max": "large"}

Call = namedtuple("Call", "entry shape ids opt", defaults=("",))


def lpr_of(k):
    return gf.CLASS_OF.get(k, (16,))[0]  # (k = 20: the class of 32)


def chunked(k):
    return gf.CLASS_OF.get(k, (16, 2, 1))[2] > 1


def fixed_order(k, hot):
    """grad_forms_common.fixed_order for the factor counts its table does not list as well."""
    return hot in (-1, -2) or chunked(k)


def host_sizes(k, n_cu=256, capped=None):
    """The batch sizes the names stand for on a device of `n_cu` compute units (forward_form of
    rfm_fm.hip, restated: the host test needs numbers, the GPU tests ask the library).  `capped`: a
    max_batch below the second trip (k = 400: 3 000)."""
    lpr = lpr_of(k)
    trip = 1024 // lpr * (1 if chunked(k) else 2)
    m = (n_cu // 2 - 1) * trip + 1
    if capped:
        assert m <= capped
        return {"one": 1, "group": 256 // lpr + 1, "mid": m - 1, "max": capped}
    return {"one": 1, "group": 256 // lpr + 1, "below": m - 1, "min": m, "min+1": m + 1, "trip2": n_cu * trip + 1}


def increments(call):
    """Increments of the plan's step counter by a call (see the module's docstring)."""
    return RIDE_ITERS if call.entry == "train_loss" and "ride" in call.opt else ADVANCE[call.entry]


# --------------------------------------------------------------------------
# logs
# --------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def history_log(n_rows, seed=0, content=0):
    """`n_rows` rows of 0 .. 16 entries (half of the rows at a length of EDGES), ascending columns:
    24 frequent columns (0 and 1 in every row that has room for them, column c with weight 1 - c / 26)
    and 2 000 sparse ones, so that a small batch touches only a few of those.  `content`: other
    columns and values in rows of the same lengths (what a caller writes into the same arrays)."""
    rng = np.random.default_rng(4100 + seed)
    lens = np.where(rng.random(n_rows) < 0.5, rng.choice(EDGES, size=n_rows), rng.integers(2, 17, size=n_rows))
    rng = np.random.default_rng([4100 + seed, content])
    weight = np.full(N_COLS, 0.003)
    weight[:N_FREQ] = 1.0 - np.arange(N_FREQ) / 26.0
    indptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    cols = np.empty(indptr[-1], dtype=np.int32)
    for at in range(0, n_rows, 2048):  # (weighted draws without replacement: the L smallest keys)
        ll = lens[at: at + 2048]
        keys = -np.log(rng.random((len(ll), N_COLS))) / weight[None, :]
        keys[:, 0], keys[:, 1] = -2.0, -1.0
        first = np.argsort(keys, axis=1)[:, :16]
        for L in np.unique(ll):
            if L:
                rows = np.flatnonzero(ll == L)
                cols[indptr[at + rows][:, None] + np.arange(L)[None, :]] = np.sort(first[rows, :L], axis=1)
    X = csr_matrix((rng.standard_normal(indptr[-1]), cols, indptr), shape=(n_rows, N_COLS))
    y = (rng.random(n_rows) < 0.5).astype(np.int64)
    p = rng.uniform(0.1, 1.0, size=n_rows) ** 0.5
    return {"features": X, "labels": y, "pscores": p}


def hot_mode_for(log, max_batch):
    """The hot_min_count that makes exactly the 24 frequent columns the hot class of a plan of
    `max_batch` (rfm_fm_plan.hip: a column is hot where len * max_batch >= hot_min * n_rows)."""
    n_rows = log["features"].shape[0]
    cnt = np.bincount(log["features"].indices, minlength=N_COLS).astype(np.int64)
    hot = int(cnt[:N_FREQ].min() * max_batch // n_rows)
    assert hot >= 1 and (cnt[:N_FREQ] * max_batch >= hot * n_rows).all()
    assert (cnt[N_FREQ:] * max_batch < hot * n_rows).all(), (hot, int(cnt[N_FREQ:].max()))
    return hot


@functools.lru_cache(maxsize=None)
def theta(k):
    """Parameters whose pair term matters to a row's score (forward_rows_common.forward_params)."""
    return fr.forward_params(500 + k, N_COLS, k, 8)


# --------------------------------------------------------------------------
# row ids
# --------------------------------------------------------------------------
def next_ids(rng, n_rows, size, kind, prev):
    """`size` distinct row ids related to the batch before (`prev`) as `kind` says."""
    if kind == "fresh" or prev is None:
        return rng.permutation(n_rows)[:size].astype(np.int32)
    if kind == "same":
        assert len(prev) == size, "the same ids: the same shape"
        return prev.copy()
    rest = np.setdiff1d(np.arange(n_rows, dtype=np.int32), prev)
    if kind == "disjoint":
        assert len(rest) >= size, f"no {size} rows outside the {len(prev)} of the batch before"
        return rng.permutation(rest)[:size].astype(np.int32)
    assert kind == "overlap"
    m = max(min(len(prev), max(1, size // 2)), size - len(rest))
    assert m <= len(prev)
    return rng.permutation(np.concatenate([rng.permutation(prev)[:m], rng.permutation(rest)[: size - m]])).astype(np.int32)


def resolve(seq, sizes, n_rows, seed):
    """The row ids of every call of a sequence: [iterations, rows] for the train entries (the first
    iteration related to the batch before as the call says, the others fresh), [rows] for the other
    entries, None for the entries without a batch.  "The batch before" is the last batch of the
    last call that had one."""
    rng = np.random.default_rng(9000 + seed)
    out, prev = [], None
    for c in seq:
        if c.entry in UNSHAPED:
            out.append(None)
            continue
        size = sizes[c.shape]
        ids = next_ids(rng, n_rows, size, c.ids, prev)
        if c.entry in ("train", "train_loss"):
            ids = np.stack([ids] + [next_ids(rng, n_rows, size, "fresh", None) for _ in range(increments(c) - 1)])
        out.append(ids)
        prev = ids if ids.ndim == 1 else ids[-1]
    return out


# --------------------------------------------------------------------------
# the sequences
# --------------------------------------------------------------------------
def class_of(call):
    return SHAPE_CLASS.get(call.shape)


def coverage(seqs):
    """What the sequences of a k-class cover: adjacent ordered pairs of entries; per entry the
    ordered pairs of shape classes around it -- (class of the call before, class of the call) for
    an entry with a batch, (class before, class after) for rows_empty and plan_forward; the ids
    kinds right after a trip2 / max call; per (entry, shape) the parities of the step counter
    before the call."""
    pairs, around, after_full, parity = set(), set(), set(), {}
    for seq in seqs:
        steps = 0
        for i, c in enumerate(seq):
            b = seq[i - 1] if i else None
            if b is not None:
                pairs.add((b.entry, c.entry))
                if b.shape in ("trip2", "max"):
                    after_full.add(c.ids)
                if c.entry not in UNSHAPED and class_of(b):
                    around.add((c.entry, class_of(b), class_of(c)))
                if c.entry in UNSHAPED and class_of(b) and i + 1 < len(seq) and class_of(seq[i + 1]):
                    around.add((c.entry, class_of(b), class_of(seq[i + 1])))
            if increments(c):
                parity.setdefault((c.entry, c.shape), set()).add(steps & 1)
            steps += increments(c)
    return pairs, around, after_full, parity


ALL_PAIRS = {(a, b) for a in ENTRIES for b in ENTRIES}
ALL_AROUND = {(e, a, b) for e in ENTRIES for a in ("small", "large") for b in ("small", "large")}

# The sequences, one per case: "number entry shape ids [opt]" per call.  Every one starts with the same
# 23 calls on the names of its plan -- full batch -> one row -> a last workgroup of one row -> the
# largest one-row launch -> the smallest many-rows launch; rows_empty after a full step and a rows
# call after it; the same ids twice; disjoint ids; every ids kind after a full batch; step ->
# step_ada -> grad -> step; plan_forward between two steps; both train forms next to each other.
# The chunked ones then call the same (entry, shape) at both parities of the step counter, padded by
# rows_empty, which leaves the counter alone; k16-row-records, the one plan of one chunk per lane that
# keeps row records, has the riding calls between the other entries.  The rest of each fills what
# test_plan_history_host.py asks of the sequences of a k-class together.
_TEXT = {
    "k32-lanes8": """
     0 grad trip2 fresh
     1 grad one disjoint
     2 grad min+1 overlap
     3 grad below fresh
     4 grad min fresh
     5 step trip2 fresh
     6 rows_empty zero -
     7 rows one fresh ranges
     8 step below fresh
     9 step below same
    10 rows trip2 fresh
    11 rows trip2 same
    12 rows one disjoint
    13 step trip2 fresh
    14 step_ada group overlap
    15 grad one disjoint
    16 step one same
    17 plan_forward val -
    18 step one same
    19 train one fresh
    20 train_loss one overlap
    21 train min fresh
    22 train_loss min same big
    23 step_ada min+1 overlap
    24 train below disjoint
    25 step_ada min overlap
    26 step group fresh
    27 grad trip2 overlap
    28 train min fresh
    29 grad min same
    30 step_ada below fresh
    31 train_loss min overlap big
    32 rows_empty zero -
    33 step_ada min+1 disjoint
    34 plan_forward val -
    35 step_ada below overlap
    36 rows_empty zero -
    37 grad one fresh
    38 rows_empty zero -
    39 train min+1 overlap
    40 plan_forward val -
    41 grad trip2 fresh
    42 rows one overlap ranges
    """,
    "k20-lanes8": """
     0 grad trip2 fresh
     1 grad one disjoint
     2 grad min+1 overlap
     3 grad below fresh
     4 grad min fresh
     5 step trip2 fresh
     6 rows_empty zero -
     7 rows one fresh ranges
     8 step below fresh
     9 step below same
    10 rows trip2 fresh
    11 rows trip2 same
    12 rows group disjoint
    13 step trip2 fresh
    14 step_ada one overlap
    15 grad group disjoint
    16 step group same
    17 plan_forward val -
    18 step group same
    19 train group fresh
    20 train_loss group overlap
    21 train min fresh
    22 train_loss min same big
    23 plan_forward val -
    24 rows group overlap ranges
    25 plan_forward val -
    26 train trip2 disjoint
    27 rows one overlap ranges
    28 step_ada group fresh
    29 step_ada below overlap
    30 rows one disjoint
    31 grad one same
    32 plan_forward val -
    33 rows_empty zero -
    34 rows_empty zero -
    35 plan_forward val -
    36 plan_forward val -
    37 train_loss below fresh
    38 rows one overlap ranges
    39 rows_empty zero -
    40 step group disjoint
    41 rows group same ranges
    42 train one fresh
    """,
    "k32-fixed-order": """
     0 grad trip2 fresh
     1 grad one disjoint
     2 grad min+1 overlap
     3 grad below fresh
     4 grad min fresh
     5 step trip2 fresh
     6 rows_empty zero -
     7 rows one fresh ranges
     8 step below fresh
     9 step below same
    10 rows trip2 fresh
    11 rows trip2 same
    12 rows one disjoint
    13 step trip2 fresh
    14 step_ada below overlap
    15 grad one disjoint
    16 step one same
    17 plan_forward val -
    18 step one same
    19 train one fresh
    20 train_loss one overlap
    21 train min fresh
    22 train_loss min same big
    23 rows_empty zero -
    24 train_loss group overlap big
    25 train below disjoint
    26 train below same
    27 step group fresh
    28 train below overlap
    29 rows_empty zero -
    """,
    "k32-no-hot-class": """
     0 grad trip2 fresh
     1 grad one disjoint
     2 grad min+1 overlap
     3 grad below fresh
     4 grad min fresh
     5 step trip2 fresh
     6 rows_empty zero -
     7 rows one fresh ranges
     8 step below fresh
     9 step below same
    10 rows trip2 fresh
    11 rows trip2 same
    12 rows group disjoint
    13 step trip2 fresh
    14 step_ada group overlap
    15 grad group disjoint
    16 step group same
    17 plan_forward val -
    18 step group same
    19 train group fresh
    20 train_loss group overlap
    21 train min fresh
    22 train_loss min same big
    """,
    "k16-row-records": """
     0 grad trip2 fresh
     1 grad one disjoint
     2 grad min+1 overlap
     3 grad below fresh
     4 grad min fresh
     5 step trip2 fresh
     6 rows_empty zero -
     7 rows one fresh ranges
     8 step below fresh
     9 step below same
    10 rows trip2 fresh
    11 rows trip2 same
    12 rows one disjoint
    13 step trip2 fresh
    14 step_ada group overlap
    15 grad one disjoint
    16 step one same
    17 plan_forward val -
    18 step one same
    19 train one fresh
    20 train_loss one overlap
    21 train min fresh
    22 train_loss min same big
    23 train_loss group fresh ride
    24 step group same
    25 train_loss one fresh ride
    26 rows group fresh
    27 train_loss group disjoint ride
    28 grad min fresh
    29 train_loss group fresh ride
    30 step_ada group overlap
    """,
    "k65-chunked": """
     0 grad trip2 fresh
     1 grad one disjoint
     2 grad min+1 overlap
     3 grad below fresh
     4 grad min fresh
     5 step trip2 fresh
     6 rows_empty zero -
     7 rows one fresh ranges
     8 step below fresh
     9 step below same
    10 rows trip2 fresh
    11 rows trip2 same
    12 rows one disjoint
    13 step trip2 fresh
    14 step_ada group overlap
    15 grad one disjoint
    16 step one same
    17 plan_forward val -
    18 step one same
    19 train one fresh
    20 train_loss one overlap
    21 train min fresh
    22 train_loss min same big
    23 rows_empty zero -
    24 step below fresh
    25 grad one fresh
    26 grad one same
    27 rows group fresh
    28 rows_empty zero -
    29 rows group fresh
    30 train one fresh
    31 train one fresh
    32 train_loss group fresh
    33 train_loss group fresh
    34 step_ada one fresh
    35 step_ada one same
    36 train_loss min+1 overlap big
    37 grad trip2 fresh
    38 step_ada trip2 same
    39 train group fresh
    40 step_ada trip2 overlap
    41 step one disjoint
    42 train_loss one same big
    43 rows trip2 fresh
    44 train_loss one overlap big
    45 plan_forward val -
    46 grad min+1 disjoint
    47 train min+1 same
    48 rows_empty zero -
    49 step_ada min fresh
    50 plan_forward val -
    51 step_ada group overlap
    52 rows_empty zero -
    53 grad trip2 disjoint
    54 plan_forward val -
    55 rows min overlap ranges
    56 step_ada group fresh
    57 rows below overlap ranges
    58 grad one disjoint
    59 rows_empty zero -
    60 rows_empty zero -
    61 train group overlap
    62 grad below fresh
    63 train_loss one overlap big
    """,
    "k400-sliced": """
     0 grad max fresh
     1 grad one disjoint
     2 grad max overlap
     3 grad mid fresh
     4 grad max fresh
     5 step max fresh
     6 rows_empty zero -
     7 rows one fresh ranges
     8 step mid fresh
     9 step mid same
    10 rows max fresh
    11 rows max same
    12 rows group disjoint
    13 step max fresh
    14 step_ada one overlap
    15 grad group disjoint
    16 step group same
    17 plan_forward val -
    18 step group same
    19 train group fresh
    20 train_loss group overlap
    21 train max fresh
    22 train_loss max same big
    23 rows_empty zero -
    24 step mid fresh
    25 grad one fresh
    26 grad one same
    27 rows group fresh
    28 rows_empty zero -
    29 rows group fresh
    30 train one fresh
    31 train one fresh
    32 train_loss group fresh
    33 train_loss group fresh
    34 step_ada one fresh
    35 step_ada one same
    36 rows group overlap ranges
    37 plan_forward val -
    38 rows_empty zero -
    39 train_loss mid disjoint
    40 step mid same
    41 rows_empty zero -
    42 plan_forward val -
    43 train group fresh
    44 plan_forward val -
    45 plan_forward val -
    46 train_loss mid overlap big
    47 train one disjoint
    48 step one same
    49 train mid fresh
    50 rows one overlap ranges
    """,
}


def _parse(text):
    calls = []
    for line in text.strip().splitlines():
        number, entry, shape, ids, *opt = line.split()
        assert int(number) == len(calls), line
        calls.append(Call(entry, shape, ids, " ".join(opt)))
    return tuple(calls)


# name -> (k, hot mode: "min" = the measured threshold of the 24 frequent columns, max_batch name)
CASES = {"k32-lanes8": (32, "min", "trip2"), "k20-lanes8": (20, "min", "trip2"), "k32-fixed-order": (32, -2, "trip2"),
         "k32-no-hot-class": (32, -1, "trip2"), "k16-row-records": (16, "min", "trip2"), "k65-chunked": (65, 0, "trip2"),
         "k400-sliced": (400, 0, "max")}
K400_MAX_BATCH = 3000
# two k-classes: one chunk of factors per lane (k = 32 and 20 on padded row blocks, k = 16 on row records), and
# several (two slot bitmaps by step parity, no hot class, the sliced loss forwards at k = 400)
SEQUENCES = {"one-chunk": {n: _parse(_TEXT[n]) for n in CASES if not chunked(CASES[n][0])},
             "chunked": {n: _parse(_TEXT[n]) for n in CASES if chunked(CASES[n][0])}}
SEQUENCE_OF = {name: seq for group in SEQUENCES.values() for name, seq in group.items()}


# --------------------------------------------------------------------------
# the gradient oracle on the entries of the CSR
# --------------------------------------------------------------------------
def grad_oracle(log, ids, w0, w, V):
    """grad_forms_common.fm_gradients_ld (same result tuple, same sums and magnitudes, long double)
    without the dense matrix: the rows of a batch of 30 000 rows on 2 000 columns are 250 000
    entries, not 60 million elements.  test_plan_history_host.py holds it to the dense statement."""
    X = log["features"][np.asarray(ids, dtype=np.int64)]
    indptr, cols, x = X.indptr.astype(np.int64), X.indices.astype(np.int64), X.data.astype(LD)
    m, (n, k) = X.shape[0], V.shape
    w0 = LD(np.asarray(w0, dtype=np.float64).reshape(-1)[0])
    w, V = np.asarray(w).astype(LD), np.asarray(V).astype(LD)
    length = np.diff(indptr)
    held = np.flatnonzero(length > 0)
    starts = indptr[held]
    row_of = np.repeat(np.arange(m), length)
    q, lin, sq = np.zeros((m, k), dtype=LD), np.zeros(m, dtype=LD), np.zeros(m, dtype=LD)
    if len(cols):
        vx = V[cols] * x[:, None]
        q[held] = np.add.reduceat(vx, starts, axis=0)
        lin[held] = np.add.reduceat(w[cols] * x, starts)
        sq[held] = np.add.reduceat((vx * vx).sum(axis=1), starts)
        del vx
    z = np.clip(w0 + lin + ((q * q).sum(axis=1) - sq) / 2, -LD(fr.CLIP), LD(fr.CLIP))
    e = np.asarray(log["labels"][ids]).astype(LD) / np.asarray(log["pscores"][ids]).astype(LD) - 1 / (1 + np.exp(-z))
    g_w, S_w, exx, aexx = (np.zeros(n, dtype=LD) for _ in range(4))
    G_V, S_V = np.zeros((n, k), dtype=LD), np.zeros((n, k), dtype=LD)
    if len(cols):
        order = np.argsort(cols, kind="stable")
        cs = cols[order]
        first = np.flatnonzero(np.concatenate([[True], cs[1:] != cs[:-1]]))
        uc = cs[first]
        ex = (e[row_of] * x)[order]
        g_w[uc] = -np.add.reduceat(ex, first)
        S_w[uc] = np.add.reduceat(np.abs(ex), first)
        exx[uc] = np.add.reduceat(ex * x[order], first)
        aexx[uc] = np.add.reduceat(np.abs(ex) * np.abs(x[order]), first)
        T = ex[:, None] * q[row_of[order]]
        G_V[uc] = -np.add.reduceat(T, first, axis=0)
        S_V[uc] = np.add.reduceat(np.abs(T), first, axis=0)
        del T
    G_V += exx[:, None] * V
    S_V += aexx[:, None] * np.abs(V)
    return -e.sum(), g_w, G_V, (np.abs(e).sum(), S_w, S_V)


# --------------------------------------------------------------------------
# the raw ABI calls
# --------------------------------------------------------------------------
def register_log(dev, slot, rows):
    """rfm_fm_plan_register_log as fm.py calls it; rows None: the slot holds nothing again."""
    from relevance_factorizationmachine_amd import _lib
    rt = dev.rt
    ptrs = (*rows.csr_ptrs(), rows.n_rows) if rows is not None else (None, None, None, 0)
    _lib.check(rt.lib.rfm_fm_plan_register_log(rt.ctx, dev.plan.handle, slot, *ptrs))


def train(dev, params, ids, val, lr, losses, call_iters=None, eps=fr.EPS):
    """rfm_fm_train of the batches ids [n_iters, batch] -> (train losses, validation losses), NaN-filled
    buffers with guard elements behind them (all NaN where `losses` is False: nothing may be written).
    call_iters: rfm_fm_train_part, a piece of a call of that many iterations (the same loss forms)."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    rt = dev.rt
    ids = np.ascontiguousarray(ids, dtype=np.int32)
    n_iters, batch = ids.shape
    d_ids = rt.upload(ids.reshape(-1))
    tl = torch.full((n_iters + gf.GUARD,), float("nan"), dtype=torch.float64, device=rt.torch_device)
    vl = torch.full((n_iters + gf.GUARD,), float("nan"), dtype=torch.float64, device=rt.torch_device)
    args = (rt.ctx, dev.plan.handle, *dev.log_ptrs(), d_ids.data_ptr(), batch, n_iters, *params.ptrs(), lr,
            *val.csr_ptrs(), val.y.data_ptr(), val.p.data_ptr(), val.n_rows, eps,
            tl.data_ptr() if losses else None, vl.data_ptr() if losses else None)
    _lib.check(rt.lib.rfm_fm_train(*args) if call_iters is None else rt.lib.rfm_fm_train_part(*args, call_iters))
    rt.sync()
    t, v = tl.cpu().numpy(), vl.cpu().numpy()
    assert np.isnan(t[n_iters:]).all() and np.isnan(v[n_iters:]).all(), "a loss past the iterations was written"
    return t, v


def plan_forward(dev, rows, params):
    """rfm_fm_plan_forward of every row of `rows` (a forward_rows_common.DeviceRows) into a NaN-filled
    buffer with guard elements behind it."""
    import torch
    from relevance_factorizationmachine_amd import _lib
    rt = dev.rt
    out = torch.full((rows.n_rows + gf.GUARD,), float("nan"), dtype=torch.float64, device=rt.torch_device)
    _lib.check(rt.lib.rfm_fm_plan_forward(rt.ctx, dev.plan.handle, *rows.csr_ptrs(), rows.n_rows, *params.ptrs(),
                                          out.data_ptr()))
    rt.sync()
    got = out.cpu().numpy()
    assert np.isnan(got[rows.n_rows:]).all(), "a score past the rows of the log was written"
    return got[: rows.n_rows]
