"""CPU-side checks of the C-ABI library: it loads, exports every symbol the
header declares, and its host-only entry points (sampler, MF schedule) match
NumPy / a Python restatement.  No GPU needed."""
import os
import re

import numpy as np
import pytest

from mf_step_common import levels_py as _levels_py
from relevance_factorizationmachine_amd import _lib
from relevance_factorizationmachine_amd.runtime import mf_schedule, mf_schedule_ex, sample_batches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "rfm_hip.h")).read()
    declared = sorted(set(re.findall(r"^int32_t\s+(rfm_\w+)\s*\(", header, flags=re.M)))
    assert declared, "no declarations parsed"
    assert {"rfm_fm_sliced_geometry", "rfm_fm_plan_sliced_columns"} <= set(declared)  # the host-only queries
    lib = _lib.load()
    for name in declared:
        assert hasattr(lib, name), f"{name} declared in rfm_hip.h but not exported"
    assert sorted(_lib.exported_symbols()) == declared, "ctypes table and header disagree"
    assert lib.rfm_version() == 100


def test_ctypes_table_matches_the_header_argument_by_argument():
    """Every ``int32_t rfm_*(...);`` of the header against ``SIGNATURES``: a parameter with a ``*`` is a
    pointer (``c_void_p``, ``c_char_p``, ``POINTER(..)``), the scalars are ``int32_t``, ``int64_t``,
    ``double`` and ``size_t`` themselves."""
    import ctypes as C

    header = open(os.path.join(ROOT, "include", "rfm_hip.h")).read()
    header = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    header = re.sub(r"//[^\n]*", " ", header)
    scalars = {"int32_t": C.c_int32, "int64_t": C.c_int64, "double": C.c_double, "size_t": C.c_size_t}

    def header_kind(param):
        if "*" in param:
            return "pointer"
        kinds = [name for name in scalars if re.search(r"\b%s\b" % name, param)]
        assert len(kinds) == 1, f"cannot classify parameter {param!r}"
        return kinds[0]

    def table_kind(ctype):
        for name, scalar in scalars.items():
            if ctype is scalar:
                return name
        assert ctype in (C.c_void_p, C.c_char_p) or issubclass(ctype, C._Pointer), ctype
        return "pointer"

    declared = re.findall(r"^int32_t\s+(rfm_\w+)\s*\(([^)]*)\)\s*;", header, flags=re.M)
    # (a key written twice in the dict literal is dropped silently: the count against the header catches it)
    assert len(declared) == 89 == len(_lib.SIGNATURES)
    mismatches = []
    for name, params in declared:
        params = [p.strip() for p in params.split(",") if p.strip() not in ("", "void")]
        want = [header_kind(p) for p in params]
        got = [table_kind(t) for t in _lib.SIGNATURES[name]]
        if want != got:
            mismatches.append((name, want, got))
    assert not mismatches, mismatches


@pytest.mark.parametrize("n,batch", [(1, 1), (2, 2), (7, 3), (1000, 64), (3660, 500), (43036, 2000), (65537, 100)])
def test_sampler_bit_exact_vs_numpy(n, batch):
    got = sample_batches(n, batch, 0, 5, n_threads=3)
    for e in range(5):
        order = np.arange(n)
        np.random.RandomState(e).shuffle(order)
        np.testing.assert_array_equal(got[e], order[:batch])


def test_sampler_large_and_offsets():
    n = 1_000_000
    got = sample_batches(n, 2000, 7, 2, n_threads=2)
    for i, e in enumerate((7, 8)):
        order = np.arange(n)
        np.random.RandomState(e).shuffle(order)
        np.testing.assert_array_equal(got[i], order[:2000])


def test_sampler_golden(golden):
    g = golden("batch_ids")
    for key in g.files:
        n, e = key[1:].split("_e")
        np.testing.assert_array_equal(sample_batches(int(n), 32, int(e), 1)[0], g[key])


def test_sampler_rejects_oversized_batch():
    # the reference's resample raises ValueError (sklearn) when B > N
    with pytest.raises(ValueError, match="Cannot sample 11 out of arrays with dim 10"):
        sample_batches(10, 11, 0, 1)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_mf_schedule_matches_python(seed):
    rng = np.random.default_rng(seed)
    b, nu, ni = 3000, 500, 80
    users = rng.integers(0, nu, size=b)
    items = (rng.zipf(1.3, size=b) - 1) % ni
    order, lptr = mf_schedule(users, items, nu, ni)
    lev = _levels_py(users, items)
    assert len(lptr) - 1 == lev.max() + 1
    assert sorted(order.tolist()) == list(range(b))
    for l in range(len(lptr) - 1):
        grp = order[lptr[l]:lptr[l + 1]]
        assert np.all(lev[grp] == l)
        assert np.all(np.diff(grp) > 0)  # ascending batch position
        # rows touched inside a level are disjoint
        assert len(set(users[grp].tolist())) == len(grp)
        assert len(set(items[grp].tolist())) == len(grp)
    # called twice: the per-thread scratch is reset properly
    order2, lptr2 = mf_schedule(users, items, nu, ni)
    np.testing.assert_array_equal(order, order2)
    np.testing.assert_array_equal(lptr, lptr2)


def test_mf_schedule_edges():
    order, lptr = mf_schedule(np.zeros(0, np.int32), np.zeros(0, np.int32), 4, 4)
    assert order.size == 0 and lptr.tolist() == [0]
    order, lptr = mf_schedule(np.array([1, 1, 1]), np.array([0, 2, 3]), 4, 4)
    assert order.tolist() == [0, 1, 2] and lptr.tolist() == [0, 1, 2, 3]
    with pytest.raises(ValueError):
        mf_schedule(np.array([5]), np.array([0]), 4, 4)


@pytest.mark.parametrize("seed,cap", [(0, 0), (1, 5), (2, 1000)])
def test_mf_schedule_ex_records(seed, cap):
    """Level-ordered records: same levels as the plain schedule, label/propensity
    ratio, item cache slots for the most frequent repeated items, gap to the user row's previous writer."""
    rng = np.random.default_rng(seed)
    b, nu, ni = 2500, 400, 90
    users = rng.integers(0, nu, size=b)
    items = (rng.zipf(1.3, size=b) - 1) % ni
    y = (rng.random(b) < 0.5).astype(np.float64)
    p = rng.uniform(0.1, 1.0, size=b)
    ex, lptr, cache = mf_schedule_ex(users, items, y, p, nu, ni, cap)
    order, lptr0 = mf_schedule(users, items, nu, ni)
    np.testing.assert_array_equal(lptr, lptr0)
    np.testing.assert_array_equal(ex["u"], users[order])
    np.testing.assert_array_equal(ex["i"], items[order])
    np.testing.assert_array_equal(ex["ry"], (y / p)[order])
    counts = np.bincount(items, minlength=ni)
    repeated = np.flatnonzero(counts >= 2)
    assert len(cache) == min(cap, len(repeated))
    if len(cache):
        assert counts[cache].min() >= np.sort(counts[repeated])[::-1][len(cache) - 1]
    slot_of = {int(it): c for c, it in enumerate(cache)}
    lev = _levels_py(users, items)
    last_u = {}
    early_ref = np.zeros(b, dtype=np.int32)
    for s in range(b):
        pu = last_u.get(users[s], None)
        early_ref[s] = (1 << 30) if pu is None else lev[s] - pu  # RFM_MF_NO_WRITER
        last_u[users[s]] = lev[s]
    np.testing.assert_array_equal(ex["gap"], early_ref[order])
    for rec in ex:
        it = int(rec["i"])
        want = slot_of.get(it, -1 if counts[it] == 1 else -2)
        assert rec["cslot"] == want
    # the per-thread scratch is reset: a second call gives the same answer
    ex2, _, cache2 = mf_schedule_ex(users, items, y, p, nu, ni, cap)
    np.testing.assert_array_equal(ex, ex2)
    np.testing.assert_array_equal(cache, cache2)


def test_evaluator_grouping_and_recognition():
    """Host half of the device evaluator (no GPU): the grouping equals pandas'
    groupby("user").agg(list) order, and only ValEvaluator-like objects are recognised."""
    import pandas as pd

    from oracle import cpu_ref
    from relevance_factorizationmachine_amd import evaluate

    rng = np.random.default_rng(0)
    users = rng.integers(0, 50, size=1000) * 7
    order, seg_ptr = evaluate.group_by_user(users)
    assert order.dtype == np.int32 and seg_ptr.dtype == np.int32
    slices = cpu_ref._per_user_slices(users)
    assert len(slices) == len(seg_ptr) - 1
    for g, rows in enumerate(slices):
        np.testing.assert_array_equal(order[seg_ptr[g]:seg_ptr[g + 1]], rows)
    df = pd.DataFrame({"user": users, "row": np.arange(1000)})
    grouped = df.groupby("user").agg(list)
    for g, rows in enumerate(grouped["row"]):
        np.testing.assert_array_equal(order[seg_ptr[g]:seg_ptr[g + 1]], rows)
    o0, s0 = evaluate.group_by_user(np.zeros(0, np.int64))
    assert o0.shape == (0,) and s0.tolist() == [0]

    frame = pd.DataFrame({"user": users, "item": users, "label": (users % 2), "pscore": np.full(1000, 0.5),
                          "ones_pscore": np.ones(1000)})

    class Val:
        k, metric_name, interaction_df = 5, "DCG", frame
        rfm_device_evaluator = True

    u, y, p, k = evaluate.recognise(Val(), "IPS")
    assert k == 5 and p[0] == 0.5 and u.shape == (1000,) and y.sum() == (users % 2).sum()
    assert evaluate.recognise(Val(), "Naive")[2][0] == 1.0
    Val.metric_name = "Recall"
    assert evaluate.recognise(Val(), "IPS") is None
    assert evaluate.recognise(object(), "IPS") is None
    # whose evaluate() is it?  Only the reference's own (class ValEvaluator of a module
    # called evaluate), or an object that opts in, takes the device path: a subclass that
    # overrides evaluate() keeps its host callback
    import types
    mod = types.ModuleType("utils.evaluate")
    exec("class ValEvaluator:\n    k = 5\n    metric_name = 'DCG'\n"
         "    def evaluate(self, y_scores, estimator):\n        return 0.0\n", mod.__dict__)
    ref_like = mod.ValEvaluator()
    ref_like.interaction_df = frame
    assert evaluate.known_implementation(ref_like) and evaluate.recognise(ref_like, "IPS") is not None

    class Custom(mod.ValEvaluator):
        def evaluate(self, y_scores, estimator):
            return 1.0

    sub = Custom()
    sub.interaction_df = frame
    assert not evaluate.known_implementation(sub) and evaluate.recognise(sub, "IPS") is None
    assert evaluate.recognise(sub, "IPS", any_implementation=True) is not None

    class Inherits(mod.ValEvaluator):
        pass

    inh = Inherits()
    inh.interaction_df = frame
    assert evaluate.recognise(inh, "IPS") is not None


def test_csr_cache_fingerprint_follows_in_place_edits():
    from scipy.sparse import random as sprandom

    from relevance_factorizationmachine_amd.runtime import CsrCache

    X = sprandom(500, 40, density=0.1, format="csr", random_state=np.random.default_rng(0))
    a = CsrCache._fingerprint(X)
    assert a == CsrCache._fingerprint(X)
    X.data[0] += 1.0
    assert a != CsrCache._fingerprint(X)
    b = CsrCache._fingerprint(X)
    X.indices[-1] = (X.indices[-1] + 1) % 40
    assert b != CsrCache._fingerprint(X)


def test_host_tie_resolution_equals_reference_val_evaluator():
    """The host half of the device evaluator against the value the reference's own
    ValEvaluator returned on fixture G7 (stored by tests/golden/make_golden.py): with 10 % of
    the scores tied at 1.0 -- the case whose ranking NumPy's unstable sort decides -- redoing
    users with ``ValFrame.host_user_value`` gives the reference's value exactly, and so does
    the oracle's restatement of that evaluator; an evaluator under the reference's class and
    module names is recognised, and its frame is not touched."""
    import pandas as pd

    from oracle import cpu_ref
    from relevance_factorizationmachine_amd import evaluate

    names = ("user", "item", "label", "pscore", "ones_pscore")

    class ValEvaluator:
        """The reference's ValEvaluator as ``recognise`` sees it (``utils/evaluate.py``:
        class and module name, constructor arguments), the oracle's restatement as evaluate()."""

        __module__ = "utils.evaluate"
        __qualname__ = "ValEvaluator"

        def __init__(self, interaction_df, features, k, metric_name):
            self.interaction_df, self.features, self.k, self.metric_name = interaction_df, features, k, metric_name

        def evaluate(self, y_scores, estimator):
            frame = {c: self.interaction_df[c].to_numpy() for c in names}
            return cpu_ref.val_dcg(frame, y_scores, estimator, k=self.k)

    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "val_dcg.npz"))
    cols = {c: g[c] for c in names}
    ev = ValEvaluator(interaction_df=pd.DataFrame(cols), features={}, k=5, metric_name="DCG")
    assert evaluate.known_implementation(ev)
    before = ev.interaction_df.copy()
    for est, pcol in (("IPS", "pscore"), ("Naive", "ones_pscore")):
        users, labels, pscores, k = evaluate.recognise(ev, est)
        np.testing.assert_array_equal(pscores, cols[pcol])
        frame = evaluate.ValFrame(users, labels, pscores, k)
        n = frame.n_segments
        # as if the device had flagged every counted user as order dependent
        counted = np.array([frame.h_labels[frame.h_seg_ptr[u]:frame.h_seg_ptr[u + 1]].sum() != 0 for u in range(n)])
        scratch = np.concatenate([np.zeros(n), counted.astype(np.float64), counted.astype(np.float64)])
        got = frame.resolve(g["scores"], scratch)
        assert got == ev.evaluate(y_scores=g["scores"], estimator=est) == float(g[f"val_dcg_{est}"])
    pd.testing.assert_frame_equal(ev.interaction_df, before)


def test_content_hash_reads_every_byte_and_ignores_the_thread_count():
    """rfm_hash_bytes (what the upload caches compare before they trust a device copy): any
    single-byte change anywhere moves the hash, the thread count does not."""
    import ctypes as C

    lib = _lib.load()

    def h(arr, threads):
        out = C.c_uint64(0)
        a = np.ascontiguousarray(arr)
        _lib.check(lib.rfm_hash_bytes(a.ctypes.data, a.nbytes, threads, C.byref(out)))
        return out.value

    rng = np.random.default_rng(3)
    for nbytes in (0, 1, 7, 8, 31, 32, 33, 1 << 20, (1 << 20) + 5, 5 * (1 << 20) + 123):
        buf = rng.integers(0, 256, size=nbytes, dtype=np.uint8)
        base = h(buf, 1)
        assert all(h(buf, t) == base for t in (2, 3, 8, 64))
        for pos in sorted({0, nbytes // 3, nbytes // 2, max(nbytes - 9, 0), nbytes - 1} & set(range(nbytes))):
            edited = buf.copy()
            edited[pos] ^= 1
            assert h(edited, 4) != base, (nbytes, pos)
        if nbytes:
            assert h(buf[:-1], 4) != base  # the length counts
    # a 1 M-row label vector with ONE flipped label (the case a sampled fingerprint missed)
    labels = (rng.random(1_000_000) < 0.5).astype(np.int64)
    before = h(labels, 8)
    labels[123_457] = 1 - labels[123_457]
    assert h(labels, 8) != before
    from relevance_factorizationmachine_amd.runtime import content_hash
    assert content_hash(labels) == h(labels, 8)
