"""What the tests of MF fold-in (fold_in_common.py) and of FM fold-in (fm_fold_common.py) share: the
grouped examples of a case and the draws behind them, the constants of the launch shape both kernels
have, the oracle computed once per listed case, the "these inputs kept their bits" epilogue of the raw
ABI wrappers, and the small helpers of the two GPU test files.  The semantics, the case lists and the
tolerances (with their derivations) stay with their module.  Importing this module touches neither the
GPU nor the library under test."""
import functools
import zlib
from dataclasses import dataclass

import numpy as np

import mf_step_common as ms

LD = np.longdouble

FOLD_BLOCK = 256                      # rfm_mf.hip kMfBlock, rfm_fm_fold.hip kFmFoldBlock
GRID_PER_CU = 8                       # rfm_fold.hpp kFoldPerCu
N_FIXED = 23                          # rows of the fixed side of every listed case


def _sigmoid(z, dtype):
    clip = dtype(ms.LOGIT_CLIP)
    return 1 / (1 + np.exp(-np.clip(z, -clip, clip)))


def _chains(name, lengths, n_fixed=N_FIXED, lo=0):
    rng = np.random.default_rng(zlib.crc32(("ids-" + name).encode()))
    return [rng.integers(lo, n_fixed, size=int(n)) for n in lengths]


@dataclass
class FoldCaseBase:
    name: str
    k: int
    chains: list                         # per new row: the fixed-side rows of its examples, in order
    n_passes: int
    with_init: bool = False
    n_fixed: int = N_FIXED
    clip: bool = False                   # fixed rows 0 / 1 carry a bias (MF) / linear term (FM) of +900 / -900

    @property
    def n_new(self):
        return len(self.chains)

    @property
    def lengths(self):
        return np.asarray([len(c) for c in self.chains], dtype=np.int64)

    @property
    def row_ptr(self):
        return np.concatenate([[0], np.cumsum(self.lengths)]).astype(np.int64)

    @property
    def ids(self):
        return (np.concatenate(self.chains) if self.n_new else np.zeros(0)).astype(np.int32)

    @property
    def order(self):
        """New rows by descending example count, stable: what the host hands the kernel."""
        return np.argsort(-self.lengths, kind="stable").astype(np.int32)

    def _rng(self, tag=""):
        return np.random.default_rng(zlib.crc32((tag + self.name).encode()))

    def yp(self):
        """(label, propensity) of every example in row order, drawn as the parity tests draw them."""
        rng, n = self._rng(), int(self.lengths.sum())
        return (rng.random(n) < 0.5).astype(np.float64), rng.uniform(0.1, 1.0, size=n) ** 0.5

    def ry(self):
        y, p = self.yp()
        return y / p

    def data(self, side="user", interleaved=False):
        """The case as the dictionary ``fold_in_users`` (``side`` "item": ``fold_in_items``) takes.
        ``interleaved``: the rows' examples take turns (each row's own order is kept)."""
        y, p = self.yp()
        new = np.repeat(np.arange(self.n_new), self.lengths)
        pos = np.concatenate([np.arange(n) for n in self.lengths]) if self.n_new else np.zeros(0, np.int64)
        take = np.lexsort((new, pos)) if interleaved else np.arange(len(new))
        cols = (new, self.ids.astype(np.int64)) if side == "user" else (self.ids.astype(np.int64), new)
        return {"features": np.stack(cols, axis=1)[take], "labels": y[take], "pscores": p[take]}


def cached_oracle(fold_cases, fold_all):
    """``oracle(case)`` of a module: ``fold_all(case)`` in long double, computed once per case of the
    module's list ``fold_cases()``."""
    @functools.lru_cache(maxsize=None)
    def by_name(name):
        return fold_all(fold_cases()[name])

    def oracle(case):
        return by_name(case.name) if case.name in fold_cases() else fold_all(case)
    return oracle


# --------------------------------------------------------------------------
# around the raw ABI calls
# --------------------------------------------------------------------------
def upload_ints(rt, case):
    """Device copies of ``row_ptr, ids, order`` (an empty array goes up as one zero)."""
    return [rt.upload(a if a.size else np.zeros(1, a.dtype)) for a in (case.row_ptr, case.ids, case.order)]


def assert_inputs_kept(case, floats, ints):
    """After a call: every ``(Guarded, host array, what)`` of ``floats`` keeps its bits (and its
    sentinels), and so do the three arrays of ``upload_ints``."""
    for dev, host, what in floats:
        np.testing.assert_array_equal(dev.host().view(np.uint64), np.ascontiguousarray(host).view(np.uint64),
                                      err_msg=f"{case.name}: {what} changed")
    for dev, host in zip(ints, (case.row_ptr, case.ids, case.order)):
        np.testing.assert_array_equal(dev.cpu().numpy()[: host.size], host)


# --------------------------------------------------------------------------
# helpers of test_gpu_fold_in.py and test_gpu_fm_fold.py
# --------------------------------------------------------------------------
def _n_cu(rt):
    import torch
    return int(torch.cuda.get_device_properties(rt.device).multi_processor_count)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _twice(run):
    first, second = run(), run()
    for a, b in zip(first, second):
        np.testing.assert_array_equal(_bits(a), _bits(b), err_msg="two calls from the same start differ")
    return first


def _names(prefix, cases):
    return [n for n in cases if n.startswith(prefix)]
