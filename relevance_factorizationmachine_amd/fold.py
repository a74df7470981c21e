"""The host side of fold-in that ``mf.py`` and ``fm.py`` share: the grouped
examples as ``rfm_mf_fold_in`` / ``rfm_fm_fold_in`` take them, the check of a caller's initial state,
and the upload of the examples.  Host only until ``upload_examples``."""
from __future__ import annotations

import numpy as np


def fold_examples(data: dict, n_new: int, n_fixed: int, new_col: int, n_passes: int):
    """The examples of a fold-in call as ``rfm_mf_fold_in`` takes them (host only): ``data`` as
    ``fit()`` takes it, column ``new_col`` of ``features`` holding new-row indices 0..n_new-1 and the
    other column known ids 0..n_fixed-1.  Returns ``(row_ptr int64 [n_new+1], ids int32, ry float64,
    order int32 [n_new])``: the examples grouped by new row with a stable sort (a row's examples
    keep their input order), ``ry`` = label / propensity as ``fit()`` divides them, and the new rows
    by descending example count (stable) -- the order in which lane groups take them."""
    pairs = np.asarray(data["features"])
    if pairs.ndim != 2 or pairs.shape[1] < 2:
        raise ValueError("MF features must be an (N, 2) array of [user, item]")
    labels, pscores = np.asarray(data["labels"]), np.asarray(data["pscores"])
    if not (labels.ndim == pscores.ndim == 1 and labels.shape[0] == pscores.shape[0] == pairs.shape[0]):
        raise ValueError(f"{pairs.shape[0]} pairs, {labels.shape[0] if labels.ndim else 0} labels and "
                         f"{pscores.shape[0] if pscores.ndim else 0} pscores: one of each per example")
    n_new, n_passes = int(n_new), int(n_passes)
    if n_new < 0 or n_passes < 0:
        raise ValueError(f"n_new={n_new}, n_passes={n_passes}: neither may be negative")
    new, other = pairs[:, new_col].astype(np.int64), pairs[:, 1 - new_col].astype(np.int64)
    names = ("user", "item")
    if new.size:
        if new.min() < 0 or new.max() >= n_new:
            raise IndexError(f"new {names[new_col]} index out of range")
        if other.min() < 0 or other.max() >= n_fixed:
            raise IndexError(f"{names[1 - new_col]} id out of range")
    by_row = np.argsort(new, kind="stable")
    counts = np.bincount(new, minlength=n_new)
    row_ptr = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    ry = (labels.astype(np.float64) / pscores.astype(np.float64))[by_row]
    order = np.argsort(-counts, kind="stable").astype(np.int32)
    return row_ptr, other[by_row].astype(np.int32), ry, order


def initial_state(init, n_new: int, n_factors: int, names):
    """``init`` of a fold-in call as two float64 host arrays ``([n_new, n_factors], [n_new])``, or
    None for a cold start.  ``names``: what the model calls the two, for the ``ValueError``."""
    if init is None:
        return None
    rows, bias = (np.asarray(a, dtype=np.float64) for a in init)
    if rows.shape != (n_new, n_factors) or bias.shape != (n_new,):
        raise ValueError(f"init must be ({names[0]} [{n_new}, {n_factors}], {names[1]} [{n_new}]), got {rows.shape}, "
                         f"{bias.shape}")
    return rows, bias


def upload_examples(rt, row_ptr, ids, ry, order):
    """Device copies of what ``fold_examples`` returned, in the order the two entries take their
    pointers; an empty array goes up as one zero, so that every pointer is valid.  The caller holds
    the tensors until its launch is enqueued."""
    return [rt.upload(a if a.size else np.zeros(1, a.dtype)) for a in (row_ptr, ids, ry, order)]
