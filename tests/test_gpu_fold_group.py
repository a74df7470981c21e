"""Fold-in examples grouped on the device -- rfm_fold_group through the raw C ABI and
``fold.group_examples_device`` against ``fold.fold_examples`` on the same data, and fold_in_users /
fold_in_items of both models with the log on the device against the same call with the log on the host.
Needs an MI355X: ``pytest -m gpu``.

There is no tolerance anywhere: ``row_ptr``, ``ids``, ``ry`` and ``order`` must equal the host's in dtype
and value, ``ry`` in bits, and the folded rows / columns must have the bits of the host-grouped call (both
fold kernels are order-deterministic).  Every output of the raw call lies between sentinels, starts as
sentinels (so what is not to be written is seen to be left alone), every input keeps its bits, and every
call is made twice with equal results.  Every case asserts the path and the grid it means from
rfm_fold_group_geometry.

On the code before N18 every test here fails: the entries and the keywords do not exist."""
import numpy as np
import pytest

import fm_fold_common as fmc
import fold_group_common as gc
import fold_in_common as fc
from fold_common import _bits, _n_cu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rt():
    from relevance_factorizationmachine_amd import runtime
    return runtime.Runtime.get()


@pytest.fixture(scope="module")
def cases(rt):
    return gc.group_cases(_n_cu(rt))


def _geometry(rt, case):
    """The two groupings of a case: the examples into rows, the rows into counts."""
    from relevance_factorizationmachine_amd import fold
    g1, g2 = fold.group_geometry(rt, case.n, case.n_new), fold.group_geometry(rt, case.n_new, case.n + 1)
    assert g1 == gc.geometry_py(case.n, case.n_new, _n_cu(rt)) and g2 == gc.geometry_py(case.n_new, case.n + 1, _n_cu(rt))
    assert g1["cap"] == gc.CAP
    return g1, g2


def _check(rt, case, **how):
    got, status, kept = gc.run_group(rt, case, **how)
    gc.assert_same(got, gc.want_of(case), case.name)
    assert status.tolist() == [0, 0, -1, 0] and kept == case.n
    return got


# --------------------------------------------------------------------------
# a. the edges: nothing to do, one example, one row around the LDS cap in either pass
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["n0", "n0-nnew0", "n1"])
def test_nothing_and_one(rt, cases, name):
    got = _check(rt, cases[name])
    if name == "n0":
        assert got[0].tolist() == [0] * 6 and got[3].tolist() == [0, 1, 2, 3, 4]


def test_no_rows_leaves_everything_but_row_ptr_and_status(rt):
    """n_new == 0 with examples (all of them out of range, then): nothing but the zeroing is enqueued."""
    case = gc._case("nnew0-examples", [0, 0, 1], 0)
    got, status, kept = gc.run_group(rt, case)
    assert got[0].tolist() == [0] and kept == 0 and status.tolist() == [0, 0, -1, 0]


@pytest.mark.parametrize("n", [gc.CAP - 1, gc.CAP, gc.CAP + 1])
def test_one_row_around_the_cap(rt, cases, n):
    case = cases[f"one-row-{n}"]
    g1, g2 = _geometry(rt, case)
    # the row is one bin of n in the first grouping: LDS up to the cap, the walk beyond it
    assert g1["cap"] == gc.CAP and g1["mid_grid"] >= 1 and g1["long_grid"] == (1 if n > gc.CAP else 0)
    assert g2["mid_grid"] == 0 and g2["long_grid"] == 0
    _check(rt, case)


def test_long_bin_in_the_order_pass(rt, cases):
    case = cases["reversed-singles"]
    g1, g2 = _geometry(rt, case)
    assert case.n_new == g2["cap"] + 1 and g2["long_grid"] == 1        # every row has one example: one bin of cap + 1 rows
    got = _check(rt, case)
    np.testing.assert_array_equal(got[3], np.arange(case.n_new))


@pytest.mark.parametrize("name", ["empty-rows", "equal-counts"])
def test_empty_rows_and_equal_counts(rt, cases, name):
    got = _check(rt, cases[name])
    if name == "equal-counts":
        np.testing.assert_array_equal(got[3], np.arange(cases[name].n_new))


# --------------------------------------------------------------------------
# b. a log-normal log: every tier at once; more bins than one turn of the per-bin grid
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["lognormal", "lognormal-interleaved"])
def test_lognormal_log(rt, cases, name):
    case = cases[name]
    g1, _ = _geometry(rt, case)
    lengths = np.bincount(case.data["features"][:, 0], minlength=case.n_new)
    assert (lengths > g1["cap"]).any() and ((lengths > g1["wave_cap"]) & (lengths <= g1["cap"])).any()
    assert g1["mid_grid"] >= 1 and g1["long_grid"] >= 1 and g1["key_grid"] > 1
    _check(rt, case)


def test_more_bins_than_one_turn_of_the_grid(rt, cases):
    case = cases["many-bins"]
    g1, _ = _geometry(rt, case)
    assert g1["bin_grid"] == _n_cu(rt) * gc.PER_CU and case.n_new == g1["bin_grid"] * gc.WAVES + 37
    _check(rt, case)


# --------------------------------------------------------------------------
# c. ids of 4 and 8 bytes, strides 1 and 2, both columns; labels and propensities
# --------------------------------------------------------------------------
@pytest.mark.parametrize("layout", ["rows", "columns"])
@pytest.mark.parametrize("id_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("name", ["mixed", "mixed-items"])
def test_id_width_stride_and_column(rt, cases, name, id_dtype, layout):
    _check(rt, cases[name], id_dtype=id_dtype, layout=layout, workspace_extra=64)


def test_inexact_quotients_have_the_hosts_bits(rt, cases):
    _check(rt, cases["inexact"])


def _wrapper(rt, data, case, **kw):
    from relevance_factorizationmachine_amd import fold
    out = fold.group_examples_device(rt, data, case.n_new, case.n_fixed, case.new_col, **kw)
    rt.sync()
    return tuple(t.cpu().numpy() for t in out[:4]), out[4].cpu().numpy()


@pytest.mark.parametrize("labels", ["int64", "float32", "bool"])
def test_wrapper_label_dtypes_and_placements(rt, cases, labels):
    """Labels of an integer type and float32 propensities are converted on the device; the pieces of
    ``data`` may lie on either side, the ids in any strides."""
    import torch
    case = cases["mixed"]
    data = dict(case.data)
    data["labels"] = data["labels"].astype(labels)
    if labels == "float32":
        data["pscores"] = data["pscores"].astype(np.float32)
    want = gc.want_of(gc.types.SimpleNamespace(**{**vars(case), "data": data}))
    dev = gc.on_device(rt, data)
    dev32 = {**dev, "features": dev["features"].to(torch.int32)}
    columns = {**dev, "features": dev["features"].t().contiguous().t()}            # element stride 1
    wide = {**dev, "features": torch.cat([dev["features"], dev["features"]], dim=1)}  # (N, 4): stride 4
    mixed = {"features": dev["features"], "labels": data["labels"], "pscores": dev["pscores"]}
    assert columns["features"].stride(0) == 1 and wide["features"].stride(0) == 4
    for what, d in (("host", data), ("device", dev), ("int32", dev32), ("columns", columns), ("wide", wide), ("mixed", mixed)):
        got, status = _wrapper(rt, d, case)
        gc.assert_same(got, want, f"{labels} {what}")
        assert status.tolist() == [0, 0, -1, 0]


def test_wrapper_on_empty_logs(rt, cases):
    for name in ("n0", "n0-nnew0"):
        case = cases[name]
        got, _ = _wrapper(rt, case.data, case)
        want = gc.want_of(case)
        # (an empty array comes back as one element, as upload_examples sends it)
        np.testing.assert_array_equal(got[0], want[0])
        np.testing.assert_array_equal(got[3][: case.n_new], want[3])


# --------------------------------------------------------------------------
# d. ids out of range: counted, left out, raised or not
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(gc.bad_id_cases()))
def test_ids_out_of_range(rt, name):
    from relevance_factorizationmachine_amd import fold
    case = gc.bad_id_cases()[name]
    kept_data = gc.filtered(case.data, case.n_new, case.n_fixed, case.new_col)
    want = fold.fold_examples(kept_data, case.n_new, case.n_fixed, case.new_col, 1)
    _, want_status = gc.fold_group_np(case.data, case.n_new, case.n_fixed, case.new_col)
    for id_dtype in (np.int32, np.int64):
        got, status, kept = gc.run_group(rt, case, id_dtype=id_dtype)
        gc.assert_same(got, want, name)
        assert status.tolist() == want_status.tolist() and kept == len(want[1]) < case.n
    assert want_status[2] == (3 if name == "bad-both" else 0)
    message = "new (user|item) index out of range" if case.which == "new" else "(user|item) id out of range"
    with pytest.raises(IndexError, match=message) as dev:
        fold.group_examples_device(rt, gc.on_device(rt, case.data), case.n_new, case.n_fixed, case.new_col)
    with pytest.raises(IndexError) as host:
        fold.fold_examples(case.data, case.n_new, case.n_fixed, case.new_col, 1)
    assert str(dev.value) == str(host.value)
    got, status = _wrapper(rt, gc.on_device(rt, case.data), case, check=False)
    assert status.tolist() == want_status.tolist()
    n_kept = int(got[0][-1])
    gc.assert_same((got[0], got[1][:n_kept], got[2][:n_kept], got[3]), want, f"{name} unchecked")


def test_bad_arguments(rt, cases):
    import torch
    from relevance_factorizationmachine_amd import _lib, fold
    case = cases["mixed"]
    dev = gc.on_device(rt, case.data)
    n_bytes = fold.group_workspace(case.n, case.n_new)
    ws = rt.empty((n_bytes,), torch.uint8)
    out = [gc.Fenced(rt, case.n_new + 1, np.int64), gc.Fenced(rt, case.n, np.int32), gc.Fenced(rt, case.n, np.float64),
           gc.Fenced(rt, case.n_new, np.int32), gc.Fenced(rt, 4, np.int32)]

    def call(n=case.n, n_new=case.n_new, n_fixed=case.n_fixed, stride=2, width=8, ws_bytes=n_bytes, shift=0, null=()):
        p = {"new": dev["features"].data_ptr() + shift, "other": dev["features"].data_ptr() + 8, "labels": dev["labels"].data_ptr(),
             "pscores": dev["pscores"].data_ptr(), "ws": ws.data_ptr(), **{i: o.ptr for i, o in enumerate(out)}}
        p = {k: (None if k in null else v) for k, v in p.items()}
        return rt.lib.rfm_fold_group(rt.ctx, p["new"], p["other"], stride, width, p["labels"], p["pscores"], n, n_new, n_fixed,
                                     p["ws"], ws_bytes, p[0], p[1], p[2], p[3], p[4])
    for kw in (dict(n=-1), dict(n=2 ** 31), dict(n_new=-1), dict(n_new=2 ** 31), dict(n_fixed=-1), dict(stride=0), dict(width=2),
               dict(width=16), dict(ws_bytes=n_bytes - 1), dict(shift=4),
               *(dict(null=(k,)) for k in ("new", "other", "labels", "pscores", "ws", 0, 1, 2, 3, 4))):
        assert call(**kw) == _lib.RFM_ERR_BAD_ARG, kw
        assert _lib.last_error(), kw
    assert call() == _lib.RFM_OK
    rt.sync()
    assert int(out[0].host()[-1]) == case.n


# --------------------------------------------------------------------------
# e. end to end: the log on the device gives the bits of the log on the host
# --------------------------------------------------------------------------
def _mf_cases(rt):
    return ["shape-k1", "passes2-k33", fc.grid_case(_n_cu(rt))]


@pytest.mark.parametrize("side", ["user", "item"])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_mf_fold_in_from_a_device_log(rt, which, side):
    case = _mf_cases(rt)[which]
    case = fc.fold_cases()[case] if isinstance(case, str) else case
    model = gc.mf_model(case, side)
    fold = model.fold_in_users if side == "user" else model.fold_in_items
    data = case.data(side, interleaved=True)
    init = case.start() if case.with_init else None
    want = fold(data, case.n_new, case.n_passes, init=init).numpy()
    assert np.asarray(want[0]).any()
    for what, d, kw in (("device log", gc.on_device(rt, data), {}), ("group=device", data, dict(group="device")),
                        ("unchecked", gc.on_device(rt, data), dict(check=False)),
                        ("group=host", data, dict(group="host"))):
        got = fold(d, case.n_new, case.n_passes, init=init, **kw).numpy()
        for name, a, b in zip(("rows", "bias"), got, want):
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"{case.name} {side} {what}: {name}")
    with pytest.raises(ValueError, match="group="):
        fold(data, case.n_new, case.n_passes, group="gpu")


def _fm_cases():
    return ["shape-k1", "passes2-k33", f"count{fmc.ASSUMED_GRID + 1}-k8"]


@pytest.mark.parametrize("side", ["user", "item"])
@pytest.mark.parametrize("name", _fm_cases())
def test_fm_fold_in_from_a_device_log(rt, name, side):
    case = fmc.fold_cases()[name]
    model, sides, new_rows = gc.fm_problem(case, side)
    fold = model.fold_in_users if side == "user" else model.fold_in_items
    data = case.data(side, interleaved=True)
    init = case.start() if case.with_init else None

    def run(d, **kw):
        f = fold(sides, new_rows, d, case.n_passes, init=init, lr=case.lr, **kw)
        return f.numpy() + (f.A.cpu().numpy(), f.L.cpu().numpy())
    want = run(data)
    assert np.asarray(want[0]).any()
    for what, d, kw in (("device log", gc.on_device(rt, data), {}), ("group=device", data, dict(group="device")),
                        ("unchecked", gc.on_device(rt, data), dict(check=False))):
        for nm, a, b in zip(("V", "w", "A", "L"), run(d, **kw), want):
            np.testing.assert_array_equal(_bits(a), _bits(b), err_msg=f"{name} {side} {what}: {nm}")


def test_fold_in_raises_the_hosts_errors_from_a_device_log(rt):
    case = fc.fold_cases()["passes2-k33"]
    model = gc.mf_model(case, "user")
    data = case.data("user")
    bad = {**data, "features": data["features"].copy()}
    bad["features"][-1, 1] = case.n_fixed
    with pytest.raises(IndexError, match="item id out of range"):
        model.fold_in_users(gc.on_device(rt, bad), case.n_new, 1)
    with pytest.raises(IndexError, match="item id out of range"):
        model.fold_in_users(bad, case.n_new, 1)
    # unchecked: the example is left out, the call is the call without it
    rest = {k: v[:-1] for k, v in data.items()}
    got = model.fold_in_users(gc.on_device(rt, bad), case.n_new, 1, check=False).numpy()
    for a, b in zip(got, model.fold_in_users(rest, case.n_new, 1).numpy()):
        np.testing.assert_array_equal(_bits(a), _bits(b))
    with pytest.raises(ValueError, match="one of each per example"):
        model.fold_in_users({**gc.on_device(rt, data), "labels": data["labels"][:-1]}, case.n_new, 1)
    with pytest.raises(ValueError, match="neither may be negative"):
        model.fold_in_users(gc.on_device(rt, data), case.n_new, -1)
