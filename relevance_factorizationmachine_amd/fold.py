"""The host side of fold-in that ``mf.py`` and ``fm.py`` share: the grouped
examples as ``rfm_mf_fold_in`` / ``rfm_fm_fold_in`` take them, the check of a caller's initial state,
and the upload of the examples.  Host only until ``upload_examples``; ``group_examples_device``
(``rfm_fold_group``) is the same grouping made on the device, for a log that already
lies there."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib

_SIDES = ("user", "item")


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


# --------------------------------------------------------------------------
# the same grouping on the device
# --------------------------------------------------------------------------
def group_geometry(rt, n: int, n_bins: int) -> dict:
    """Launch shape of one grouping of ``n`` keys into ``n_bins`` bins (``rfm_fold_group_geometry``;
    ``rfm_fold_group`` makes two: ``(n, n_new)`` and ``(n_new, n + 1)``); ``rt`` None: a device of 256
    CUs.  ``cap``: the longest bin ordered in LDS, a longer one is rebuilt by a walk over all keys."""
    out = (C.c_int32 * 8)()
    _lib.check(_lib.load().rfm_fold_group_geometry(rt.ctx if rt is not None else None, int(n), int(n_bins), out))
    keys = ("cap", "block", "bin_grid", "wave_cap", "mid_grid", "long_grid", "long_block", "key_grid")
    return dict(zip(keys, (int(v) for v in out)))


def group_workspace(n: int, n_new: int) -> int:
    """Bytes of workspace of ``rfm_fold_group`` (host only)."""
    out = C.c_int64()
    _lib.check(_lib.load().rfm_fold_group_workspace(int(n), int(n_new), C.byref(out)))
    return int(out.value)


def group_mode(data: dict, group) -> str:
    """``group=`` of the fold-in methods: "host", "device", or None = where ``data["features"]`` lies."""
    if group is None:
        return "device" if hasattr(data["features"], "data_ptr") else "host"
    if group not in ("host", "device"):
        raise ValueError(f"group={group!r}: 'host', 'device' or None")
    return group


def _on_device(rt, x, what):
    """``x`` as a tensor on the runtime's device: a host array is uploaded as it is."""
    if hasattr(x, "data_ptr"):
        if x.device != rt.torch_device:
            raise ValueError(f"{what} on {x.device}, the runtime's device is {rt.torch_device}")
        return x
    return rt.upload(np.asarray(x))


def group_examples_device(rt, data: dict, n_new: int, n_fixed: int, new_col: int, check: bool = True):
    """``fold_examples`` and ``upload_examples`` in one, on the device (``rfm_fold_group``): returns
    ``(row_ptr, ids, ry, order, status)`` as device tensors, the first four equal to what
    ``fold_examples`` gives for the same ``data``, bit for bit.  Each of ``data["features"]``,
    ``["labels"]``, ``["pscores"]`` may be a host array or a tensor on the runtime's device (ids of 4
    or 8 bytes in any strides; labels and propensities of any real dtype).  ``status`` int32 [4]:
    examples with a new-row index outside 0..n_new-1, with an id outside 0..n_fixed-1, the first such
    example (-1: none), a spare word.  ``check=True`` waits once for it and raises the
    ``IndexError`` of ``fold_examples``; ``check=False`` waits for nothing and such examples are
    left out: ``row_ptr[n_new]`` is the number kept, of ``ids`` / ``ry`` only that many are written."""
    import torch

    # (every shape error before anything touches the device)
    host = {k: data[k] if hasattr(data[k], "data_ptr") else np.asarray(data[k]) for k in ("features", "labels", "pscores")}
    pairs, labels, pscores = host["features"], host["labels"], host["pscores"]
    if pairs.ndim != 2 or pairs.shape[1] < 2:
        raise ValueError("MF features must be an (N, 2) array of [user, item]")
    n = int(pairs.shape[0])
    if not (labels.ndim == pscores.ndim == 1 and labels.shape[0] == pscores.shape[0] == n):
        raise ValueError(f"{n} pairs, {labels.shape[0] if labels.ndim else 0} labels and "
                         f"{pscores.shape[0] if pscores.ndim else 0} pscores: one of each per example")
    n_new, n_fixed = int(n_new), int(n_fixed)
    if n_new < 0:
        raise ValueError(f"n_new={n_new}: may not be negative")
    pairs, labels, pscores = (_on_device(rt, host[k], k) for k in ("features", "labels", "pscores"))
    if pairs.dtype not in (torch.int32, torch.int64):
        pairs = pairs.to(torch.int64)
    labels = labels.to(torch.float64).contiguous()
    pscores = pscores.to(torch.float64).contiguous()
    width = pairs.element_size()
    if n > 1 and pairs.stride(0) < 1:
        pairs = pairs.contiguous()
    stride = int(pairs.stride(0)) if n > 1 else 1
    col = [pairs.data_ptr() + c * int(pairs.stride(1)) * width for c in (new_col, 1 - new_col)] if n else [None, None]
    row_ptr = rt.empty((n_new + 1,), torch.int64)
    ids, ry = rt.empty((max(n, 1),), torch.int32), rt.empty((max(n, 1),), torch.float64)
    order = rt.empty((max(n_new, 1),), torch.int32)
    status = rt.empty((4,), torch.int32)
    n_bytes = group_workspace(n, n_new)
    workspace = rt.empty((n_bytes,), torch.uint8)
    _lib.check(rt.lib.rfm_fold_group(
        rt.ctx, col[0], col[1], stride, width, labels.data_ptr(), pscores.data_ptr(), n, n_new, n_fixed,
        workspace.data_ptr(), n_bytes, row_ptr.data_ptr(), ids.data_ptr(), ry.data_ptr(), order.data_ptr(),
        status.data_ptr()))
    if check:
        if n and not n_new:  # (no rows: the entry enqueues nothing, and every example is out of range)
            raise IndexError(f"new {_SIDES[new_col]} index out of range")
        bad_new, bad_other = status.cpu().numpy()[:2]  # (the one host wait)
        if bad_new:
            raise IndexError(f"new {_SIDES[new_col]} index out of range")
        if bad_other:
            raise IndexError(f"{_SIDES[1 - new_col]} id out of range")
    return row_ptr, ids[:n] if n else ids, ry[:n] if n else ry, order[:n_new] if n_new else order, status


def grouped_examples(rt, data: dict, n_new: int, n_fixed: int, new_col: int, n_passes: int, group, check: bool):
    """The examples of a fold-in call, checked and grouped where ``group`` says (``group_mode``):
    returns a function that gives the four device tensors when the launch is due.  "host":
    ``fold_examples`` now and ``upload_examples`` then, as before N18; "device":
    ``group_examples_device`` now."""
    if group_mode(data, group) == "host":
        host = fold_examples(data, n_new, n_fixed, new_col, n_passes)
        return lambda: upload_examples(rt, *host)
    if int(n_new) < 0 or int(n_passes) < 0:
        raise ValueError(f"n_new={int(n_new)}, n_passes={int(n_passes)}: neither may be negative")
    dev = list(group_examples_device(rt, data, n_new, n_fixed, new_col, check)[:4])
    return lambda: dev
