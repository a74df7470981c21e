"""A call on a USED FM plan leaves what the same call leaves as the FIRST call on a fresh plan built the
same way.  Needs an MI355X: ``pytest -m gpu``.

An rfm_fm_plan carries state from launch to launch: the step counter that stamps split columns'
partial rows and picks one of two slot bitmaps, the slot marks and Q rows, the forward workgroups'
hot-sum slabs and residual sums, the touched-row table with its sequence number, the loss rows, the
registered logs with their translations, the update rule.  The sequences of plan_history_common.py
run every entry point after every other on ONE plan, across both forward shapes, and each checked
call is compared with the same call on a fresh grad_forms_common.DeviceLog that starts from COPIES
of the parameter (and accumulator) bits the used plan's call started from.

What "the same" means:

- plans whose sums all have a fixed order (hot modes -1, -2, chunked factor counts): every output bit
  for bit -- dense gradient, record list with count, order and guard records, g_w0, owner-range
  bounds, parameters and AdaGrad accumulators after a step, scores, the losses and parameters of an
  rfm_fm_train run (lr = 2^-13);
- arrival-order hot sums (hot mode = the threshold of the 24 frequent columns): the sparse class and
  g_w0 (w0, acc_w0) bit for bit -- functions of the rows' bits alone (test_gpu_forward_lanes8.py) --
  and, at EVERY checked call, the hot columns against the long-double oracle: a gradient or a record
  within grad_tol(B) * S, an SGD step within step_excess <= 1, an AdaGrad step inside
  adagrad_common's intervals (a third of a second of host time at 30 000 rows).
  rfm_fm_train on these plans: with lr > 0 the hot columns' last bits reach every column in the
  second iteration, so nothing of a three-iteration run is a function of the rows' bits, and no
  bound of the project covers three chained steps.  The call is therefore made an iteration at a
  time (rfm_fm_train_part: the loss forms of the whole call, lr = 2^-13), and each piece is held like
  a step -- the used plan and a fresh one from copies of the bits the piece started from, sparse
  class bit for bit, hot columns within step_excess <= 1 -- with its losses against
  forward_rows_common.loss_oracle at the parameters the piece left.
  The calls of RIDE_ITERS iterations whose loss rows ride in the next step's forward (the plan of
  k = 16, which keeps row records) cannot be cut: they run whole with lr = 0, parameters keeping
  their bits, losses bit for bit those of the fresh plan and inside the loss oracle; what their
  steps leave in the plan is held by the checked calls that follow.

Every output buffer is NaN-filled before the call, with guard elements behind it."""
import functools

import numpy as np
import pytest

import adagrad_common as ac
import forward_rows_common as fr
import grad_forms_common as gf
import plan_history_common as ph
from optimizer_common import ADAGRAD, SGD

pytestmark = pytest.mark.gpu

BIG, SMALL = 1024, 256
ORACLE_ROWS = 2100   # an AdaGrad step of at most so many rows must leave some column untouched


@pytest.fixture(scope="module")
def rt():
    from relevance_factorizationmachine_amd import runtime
    return runtime.Runtime.get()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(got, want, what):
    np.testing.assert_array_equal(_bits(got), _bits(want), err_msg=what)


@functools.lru_cache(maxsize=None)
def _sizes(k, capped=None):
    from relevance_factorizationmachine_amd import runtime
    rt = runtime.Runtime.get()
    lpr = ph.lpr_of(k)
    big, m = fr.forward_geometry(rt, 1 << 22, k, True), fr.many_rows_minimum(rt, k, True)
    assert big["block"] == BIG and big["lpr"] == lpr and fr.forward_geometry(rt, m - 1, k, True)["block"] == SMALL
    group = SMALL // lpr + 1
    assert fr.forward_geometry(rt, group, k, True)["grid"] == 2
    if capped:
        assert m <= capped < big["grid"] * big["trip"]
        sizes = {"one": 1, "group": group, "mid": m - 1, "max": capped}
    else:
        sizes = {"one": 1, "group": group, "below": m - 1, "min": m, "min+1": m + 1, "trip2": big["grid"] * big["trip"] + 1}
    # (the host test checks the id generators on plan_history_common.host_sizes: its restatement of the geometry)
    assert sizes == ph.host_sizes(k, capped=capped), (sizes, ph.host_sizes(k, capped=capped))
    return sizes


@functools.lru_cache(maxsize=None)
def _row_oracle(n_rows, seed, content, k):
    return fr.row_oracle(ph.history_log(n_rows, seed, content)["features"], *ph.theta(k))


def _set_rule(dev, kind, accs=None):
    from relevance_factorizationmachine_amd import _lib
    _lib.check(ac.set_optimizer(dev, kind, accs if kind == ADAGRAD else None, ac.EPS if kind == ADAGRAD else 0.0))
    assert ac.optimizer_of(dev) == kind


class History:
    """One used plan of a case of plan_history_common.CASES, its parameters and accumulators on the
    device, and the comparison of a call on it with the same call on a fresh plan."""

    def __init__(self, rt, name):
        self.rt, self.name = rt, name
        self.k, hot, full = ph.CASES[name]
        self.sizes = _sizes(self.k, ph.K400_MAX_BATCH if full == "max" else None)
        self.max_batch = self.sizes[full]
        self.n_rows = self.max_batch + ph.EXTRA_ROWS
        self.log = ph.history_log(self.n_rows)
        self.hot_mode = ph.hot_mode_for(self.log, self.max_batch) if hot == "min" else hot
        self.fixed = ph.fixed_order(self.k, self.hot_mode)
        # (a validation log of the one-row shape, and one of the many-rows shape of the forward on the caller's arrays)
        self.vals = {"": (ph.VAL_SMALL, 1), "big": (fr.many_rows_minimum(rt, self.k, False) + 37, 2)}
        self.val = {key: fr.DeviceRows(rt, ph.history_log(n, seed)) for key, (n, seed) in self.vals.items()}
        self.params = gf.Params(rt, *ph.theta(self.k))
        self.accs = gf.Params(rt, *ac.acc_init("uniform", ph.N_COLS, self.k, self.k))
        self.rule = SGD
        self.dev = self.open()
        self.hot_cols = np.sort(self.dev.plan.hot_columns())
        self.worst, self.forms, self.checked = {}, [], 0

    def open(self):
        return gf.DeviceLog(self.rt, self.log, self.k, self.max_batch, self.hot_mode)

    def close(self):
        self.dev.close()

    def assert_kind(self):
        """The plan is the kind its case claims to exercise."""
        lay, info = self.dev.plan.layout(), self.dev.plan.info()
        lpr = ph.lpr_of(self.k)  # (k = 16: 8 lanes per row, which a row of 16 entries does not fit -- row records)
        assert lay["lanes_per_row"] == lpr and lay["longest_row"] == 16 and lay["row_blocks"] == int(lpr >= 16), lay
        assert fr.forward_geometry(self.rt, self.max_batch, self.k, True)["block"] == BIG
        hot = ph.CASES[self.name][1]
        if hot == "min":
            np.testing.assert_array_equal(self.hot_cols, np.arange(ph.N_FREQ))
            assert not self.fixed
        elif hot == -2:
            assert self.hot_cols.size > 0 and self.fixed  # (no hot class: the plan fell back to -1)
        else:
            assert self.hot_cols.size == 0 and info["split_columns"] > 0 and self.fixed, info
        assert ph.chunked(self.k) == (self.name in ph.SEQUENCES["chunked"])
        if "lanes8" in self.name:
            # what launch_forward asks of the 8-lane instantiation: arrival-order hot sums, row blocks of 16
            # entries of 16 bytes, k = 20 .. 32 in fours (a many-rows step that wants no loss then takes it)
            assert not self.fixed and lay["row_block_bytes"] == 16 * 16 and 16 < self.k <= 32 and self.k % 4 == 0, lay

    # -- one call -------------------------------------------------------------------------------
    def execute(self, dev, c, ids, params, accs, rule_before=None):
        """The call on `dev`; rule_before: the rule a fresh plan is given first (the used plan keeps
        the one its history left).  Returns what the call left, by name."""
        if rule_before is not None:
            _set_rule(dev, rule_before, accs)
        out = {}
        if c.entry in ("step", "train", "train_loss"):
            _set_rule(dev, SGD)
        if c.entry == "step":
            gf.step(dev, ids, params, ph.STEP_LR)
        elif c.entry == "step_ada":
            _set_rule(dev, ADAGRAD, accs)
            gf.step(dev, ids, params, ac.LR)
        elif c.entry == "grad":
            out["grad"] = gf.dense_grad(dev, ids, params)[0]
        elif c.entry in ("rows", "rows_empty"):
            lo = np.array([ph.N_COLS * r // 5 for r in range(5)], dtype=np.int32) if "ranges" in c.opt else None
            rec = gf.grad_rows(dev, ids if ids is not None else [], params, ph.N_COLS, lo)
            rec.assert_rest_untouched()
            out.update(count=rec.count, rec=rec.rec, gw0=rec.gw0, bounds=rec.bounds)
        elif c.entry in ("train", "train_loss"):
            losses = c.entry == "train_loss"
            val = self.val["big" if "big" in c.opt else ""]
            if losses:
                ph.register_log(dev, 0, val)
            part = ph.TRAIN_ITERS if "piece" in c.opt else None
            out["forms"] = fr.train_forms(self.rt, dev.plan, ids.shape[1], ids.shape[0], part or 0, val, val.n_rows, losses, losses)
            out["train_loss"], out["val_loss"] = ph.train(dev, params, ids, val, self.train_lr(c), losses, part)
        else:
            assert c.entry == "plan_forward"
            ph.register_log(dev, 1, self.val[""])
            out["scores"] = ph.plan_forward(dev, self.val[""], params)
        out["theta"], out["accs"] = params.host(), accs.host()
        return out

    def train_lr(self, c):
        """lr of a train entry: 2^-13 where the call can be held with it (see the module's docstring)."""
        return ph.STEP_LR if self.fixed or "piece" in c.opt else 0.0

    def run(self, i, c, ids, check=True):
        if not self.fixed and c.entry.startswith("train") and "ride" not in c.opt:
            # arrival-order hot sums: the call an iteration at a time (rfm_fm_train_part, the forms of the whole call)
            for it in range(len(ids)):
                self.run_one(f"{i}.{it}", c._replace(opt=(c.opt + " piece").strip()), ids[it: it + 1], check)
        else:
            self.run_one(i, c, ids, check)

    def run_one(self, i, c, ids, check=True):
        theta0, G0, rule0 = self.params.host(), self.accs.host(), self.rule
        got = self.execute(self.dev, c, ids, self.params, self.accs)
        self.rule = {"step": SGD, "train": SGD, "train_loss": SGD, "step_ada": ADAGRAD}.get(c.entry, rule0)
        assert ac.optimizer_of(self.dev) == self.rule
        if not check:
            return got
        fresh = self.open()
        try:
            want = self.execute(fresh, c, ids, gf.Params(self.rt, *theta0), gf.Params(self.rt, *G0), rule0)
        finally:
            fresh.close()
        self.compare(f"{self.name} call {i} {tuple(c)}", c, ids, got, want, theta0, G0)
        self.checked += 1
        return got

    # -- the comparison -------------------------------------------------------------------------
    def compare(self, what, c, ids, got, want, theta0, G0):
        k, hot = self.k, (self.hot_cols if not self.fixed else np.zeros(0, dtype=np.int64))
        cold = np.setdiff1d(np.arange(ph.N_COLS), hot)  # (every column on a plan of fixed-order sums)
        for label in ("theta", "accs"):
            (a0, a1, a2), (b0, b1, b2) = got[label], want[label]
            _same(a0, b0, f"{what}: {label} w0")
            _same(a1[cold], b1[cold], f"{what}: {label} w")
            _same(a2[cold], b2[cold], f"{what}: {label} V")
        if c.entry != "step_ada":  # (gradient mode forms g alone under any rule; SGD has no accumulators)
            for a, b in zip(got["accs"], G0):
                _same(a, b, f"{what}: an accumulator moved")
        if c.entry in ("grad", "rows", "rows_empty", "plan_forward") or c.entry.startswith("train") and not self.train_lr(c):
            for a, b in zip(got["theta"], theta0):
                _same(a, b, f"{what}: a parameter moved")
        if c.entry == "grad":
            (V1, w1, g1), (V2, w2, g2) = gf.split_grad(got["grad"], ph.N_COLS, k), gf.split_grad(want["grad"], ph.N_COLS, k)
            _same(V1[cold], V2[cold], f"{what}: G_V")
            _same(w1[cold], w2[cold], f"{what}: g_w")
            _same(g1, g2, f"{what}: g_w0")
        if c.entry in ("rows", "rows_empty"):
            assert got["count"] == want["count"], (what, got["count"], want["count"])
            r1, r2 = got["rec"], want["rec"]
            _same(r1[:, 0], r2[:, 0], f"{what}: the records' columns")
            keep = ~np.isin(r2[:, 0], hot.astype(np.float64))
            _same(r1[keep], r2[keep], f"{what}: records")
            _same(got["gw0"], want["gw0"], f"{what}: g_w0 of the records")
            if "ranges" in c.opt:
                np.testing.assert_array_equal(got["bounds"], want["bounds"], err_msg=what)
        if c.entry == "rows":
            cols = np.union1d(np.unique(self.log["features"][ids].indices), self.dev.plan.hot_columns())
            assert got["count"] == len(cols), (what, got["count"], len(cols))  # the list is this call's own
            np.testing.assert_array_equal(got["rec"][: len(cols), 0], cols.astype(np.float64), err_msg=what)
        if c.entry == "rows_empty":
            assert got["count"] == 0 and got["gw0"] == 0.0 and np.isnan(got["rec"]).all(), (what, got["count"], got["gw0"])
        if c.entry.startswith("train"):
            f, losses, piece = got["forms"], c.entry == "train_loss", "piece" in c.opt
            assert f == want["forms"], (what, f, want["forms"])
            assert f["ride"] == f["ride_val"] == int("ride" in c.opt), (what, f)
            self.forms.append((c, f))
            self.assert_forms(what, c, ids, f)
            if not piece:  # (a piece's losses follow its step: the hot columns' last bits are in them)
                _same(got["train_loss"], want["train_loss"], f"{what}: train losses")
                _same(got["val_loss"], want["val_loss"], f"{what}: validation losses")
            if losses and (piece or "ride" in c.opt):
                self.hold_losses(what, c, ids, got, got["theta"])
            n_it = len(ids)
            assert np.isnan(got["train_loss"][:n_it]).all() == (c.entry == "train"), what
            assert np.isfinite(got["val_loss"][:n_it]).all() == (c.entry == "train_loss"), what
        if c.entry == "plan_forward":
            _same(got["scores"], want["scores"], f"{what}: scores")
            n, seed = self.vals[""]
            fr.assert_scores(got["scores"], fr.row_oracle(ph.history_log(n, seed)["features"], *theta0), k, what)
        if c.entry == "step_ada":
            ac.assert_untouched_bitwise(got["theta"], got["accs"], theta0, G0, self.log["features"], ids, what,
                                        some=len(ids) <= ORACLE_ROWS)
        if hot.size and c.entry in ("step", "step_ada", "grad", "rows"):
            self.hold_hot_class(what, c.entry, ids, got, theta0, G0)
        if hot.size and "piece" in c.opt:
            self.hold_hot_class(what, "step", ids[0], got, theta0, G0)

    def assert_forms(self, what, c, ids, f):
        """The loss forwards of a train_loss call take the shapes its batch and validation log stand for."""
        if c.entry != "train_loss":
            assert f["train_block"] == f["val_block"] == f["sliced"] == f["merged"] == 0, (what, f)
            return
        batch, n_val = ids.shape[1], self.vals["big" if "big" in c.opt else ""][0]
        block = {"large": BIG, "small": SMALL}
        if ph.chunked(self.k):  # both losses in one launch where batch + validation rows take the many-rows shape
            assert f["sliced"] == int(self.name == "k400-sliced" and batch + n_val >= 4096), (what, f)
            if not f["sliced"]:
                assert f["merged"] == int(fr.forward_geometry(self.rt, batch + n_val, self.k, False)["block"] == BIG), (what, f)
        else:
            assert f["sliced"] == f["merged"] == 0, (what, f)
        if not f["sliced"] and not f["merged"]:
            assert f["train_block"] == block[ph.SHAPE_CLASS[c.shape]], (what, f)
            assert f["val_block"] == (BIG if "big" in c.opt else SMALL), (what, f)

    def hold_losses(self, what, c, ids, got, theta):
        """The losses of every iteration against the long-double oracle of the parameters they were taken at."""
        k, (n, seed) = self.k, self.vals["big" if "big" in c.opt else ""]
        vlog = ph.history_log(n, seed)
        want, tol = fr.loss_oracle(fr.row_oracle(vlog["features"], *theta), k, vlog["labels"], vlog["pscores"])
        for it, b in enumerate(ids):
            fr.assert_loss(got["val_loss"][it], want, tol, f"{what}: validation loss of iteration {it}")
            w, t = fr.loss_oracle(fr.row_oracle(self.log["features"][b], *theta), k, self.log["labels"][b], self.log["pscores"][b])
            fr.assert_loss(got["train_loss"][it], w, t, f"{what}: train loss of iteration {it}")

    def note(self, key, ratio):
        assert np.isfinite(float(ratio)), (key, ratio)
        self.worst[key] = max(self.worst.get(key, 0.0), float(ratio))

    def hold_hot_class(self, what, entry, ids, got, theta0, G0):
        """The hot columns (and with them every other element) against the long-double oracle."""
        k, hot, B = self.k, self.hot_cols, len(ids)
        oracle = ph.grad_oracle(self.log, ids, *theta0)
        o_w0, o_w, o_V, (S_0, S_w, S_V) = oracle
        tol = gf.grad_tol(B)

        def ratio(g, o, S):
            return float(np.max(np.where(S > 0, np.abs(np.asarray(g).astype(ph.LD) - o) / np.where(S > 0, tol * S, 1), 0)))

        if entry == "grad":
            gf.check_dense(got["grad"], self.dev, ids, oracle, hot, what)
            G_V, g_w, _ = gf.split_grad(got["grad"], ph.N_COLS, k)
            self.note("gradient", max(ratio(G_V[hot], o_V[hot], S_V[hot]), ratio(g_w[hot], o_w[hot], S_w[hot])))
        elif entry == "rows":
            r = got["rec"][: got["count"]]
            cols = r[:, 0].astype(np.int64)
            gf.assert_within_scale(r[:, 1: k + 1], o_V[cols], S_V[cols], tol, f"{what} G_V of the records")
            gf.assert_within_scale(r[:, k + 1], o_w[cols], S_w[cols], tol, f"{what} g_w of the records")
            gf.assert_within_scale(got["gw0"], o_w0, S_0, tol, f"{what} g_w0 of the records")
            at = np.isin(cols, hot)
            self.note("records", max(ratio(r[at, 1: k + 1], o_V[hot], S_V[hot]), ratio(r[at, k + 1], o_w[hot], S_w[hot])))
        elif entry == "step":
            for name, ex in zip(("w0", "w", "V"), gf.step_excess(got["theta"], theta0, oracle, ph.STEP_LR, B)):
                assert (ex <= 1).all(), (what, name, np.argwhere(ex > 1)[:5].tolist(), float(ex.max()))
                self.note("SGD step", ex.max())
        else:
            ac.assert_inside(got["theta"], got["accs"], theta0, G0, oracle, ac.LR, ac.EPS, B, what)
            lo, hi, _, _, _ = ac.intervals(theta0[2][hot], G0[2][hot], o_V[hot], S_V[hot], ac.LR, ac.EPS, B)
            half = (hi - lo) / 2
            self.note("AdaGrad step", np.max(np.abs(got["theta"][2][hot].astype(ph.LD) - (lo + hi) / 2) / half))

    def report(self):
        print(f"{self.name}: {self.checked} calls held to a fresh plan; worst |error| / bound of the hot class: "
              + (", ".join(f"{key} {v:.3g}" for key, v in sorted(self.worst.items())) or "none (every bit compared)"))


# --------------------------------------------------------------------------
# 1. the sequences: every call against a fresh plan
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ph.CASES))
def test_every_call_of_the_sequence_leaves_what_a_fresh_plan_leaves(rt, name):
    seq = ph.SEQUENCE_OF[name]
    h = History(rt, name)
    try:
        h.assert_kind()
        for i, (c, ids) in enumerate(zip(seq, ph.resolve(seq, h.sizes, h.n_rows, 0))):
            if ids is not None:  # the launch the call's name stands for
                want = BIG if ph.SHAPE_CLASS[c.shape] == "large" else SMALL
                assert fr.forward_geometry(rt, ids.shape[-1], h.k, True)["block"] == want, (c, ids.shape)
            h.run(i, c, ids)
        h.report()
        seen = [f for c, f in h.forms if c.entry == "train_loss"]  # (History.assert_forms pins each call's)
        if name == "k400-sliced":  # the sliced loss forward with its translated validation log
            assert {f["sliced"] for f in seen} == {0, 1}, seen
        elif name == "k65-chunked":
            assert {f["merged"] for f in seen} == {0, 1}, seen
        else:
            assert {(f["train_block"], f["val_block"]) for f in seen if not f["ride"]} >= {(SMALL, SMALL), (BIG, BIG)}, seen
        assert any(f["ride_val"] for f in seen) == (name == "k16-row-records"), seen
        if not h.fixed:
            assert {"gradient", "records", "SGD step", "AdaGrad step"} <= set(h.worst), h.worst
    finally:
        h.close()


# --------------------------------------------------------------------------
# 2. the rule of the plan between steps
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k32-lanes8", "k65-chunked"])
def test_switching_the_rule_between_steps(rt, name):
    """step -> step_ada -> grad -> step at a small and at the full batch: grad under AdaGrad forms g alone,
    step and grad leave the accumulators their bits, step_ada leaves the columns outside the batch
    theirs (History.compare asserts all three for every call)."""
    full = ph.CASES[name][2]
    seq = [ph.Call("step", full, "fresh"), ph.Call("step_ada", "group", "disjoint"), ph.Call("grad", "group", "same"),
           ph.Call("step", "group", "same"), ph.Call("step_ada", full, "fresh"), ph.Call("grad", "one", "overlap"),
           ph.Call("step", full, "fresh")]
    h = History(rt, name)
    try:
        h.assert_kind()
        G = [h.accs.host()]
        for i, (c, ids) in enumerate(zip(seq, ph.resolve(seq, h.sizes, h.n_rows, 1))):
            h.run(i, c, ids)
            G.append(h.accs.host())
        moved = [any(not np.array_equal(a, b) for a, b in zip(G[i], G[i + 1])) for i in range(len(seq))]
        assert moved == [c.entry == "step_ada" for c in seq], moved
        h.report()
    finally:
        h.close()


# --------------------------------------------------------------------------
# 3. many calls: the touched-row sequence number and the step counter far from their first values
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k32-lanes8", "k65-chunked"])
def test_the_last_two_of_many_record_lists(rt, name):
    seq = [ph.Call("rows", ("one", "below")[i % 2], "fresh", "ranges" if i % 3 == 0 else "") for i in range(44)]
    h = History(rt, name)
    try:
        h.assert_kind()
        for i, (c, ids) in enumerate(zip(seq, ph.resolve(seq, h.sizes, h.n_rows, 2))):
            h.run(i, c, ids, check=i >= len(seq) - 2)
        assert h.checked == 2
        h.report()
    finally:
        h.close()


# --------------------------------------------------------------------------
# 4. registered logs: the same device arrays with other contents
# --------------------------------------------------------------------------
def _overwrite(rows, log):
    """Other contents (rows of the same lengths) into the device arrays of a DeviceRows."""
    X = log["features"]
    rows.csr.indices.copy_(rows.rt.upload(X.indices.astype(np.int32)))
    rows.csr.values.copy_(rows.rt.upload(X.data.astype(np.float64)))
    rows.y.copy_(rows.rt.upload(log["labels"], dtype=np.float64))
    rows.p.copy_(rows.rt.upload(log["pscores"], dtype=np.float64))


CONTENT_CASES = {
    # name: (k, rows of the training log, max_batch, batch, iterations, rows of the validation log, forms expected)
    "k400-sliced": (400, 4397, 3000, 3000, 3, 4200, {"sliced": 1}),
    "k128-riding": (128, 900, 600, 64, ph.RIDE_ITERS, ph.VAL_SMALL, {"sliced": 0, "ride": 1, "ride_val": 1}),
    "k128-too-large-to-ride": (128, 900, 600, 64, ph.RIDE_ITERS, 4200, {"sliced": 0, "ride": 1, "ride_val": 0}),
}


@pytest.mark.parametrize("name", sorted(CONTENT_CASES))
def test_a_registered_log_with_other_contents_in_the_same_arrays(rt, name):
    """rfm_fm_plan_register_log as fm.py calls it, then rfm_fm_train with both losses (lr = 0, so that the
    oracle of the parameters holds for every iteration) and rfm_fm_plan_forward:

    1. contents A registered: the losses and scores of A;
    2. contents B written into the SAME arrays and registered again: those of B -- nothing of A's
       translation (sliced forwards) or records (validation rows riding in the step's forward);
    3. B again WITHOUT registering: include/rfm_hip.h promises that calls naming the same three
       pointers and row count reuse what the slot holds -- the bits of run 2;
    4. other arrays (contents C) without registering: translated per call, the losses of C;
    5. the registered arrays again, still not registered anew: the bits of run 2 once more."""
    k, n_train, max_batch, batch, n_iters, n_val, expect = CONTENT_CASES[name]
    log, th = ph.history_log(n_train), ph.theta(k)
    logs = [ph.history_log(n_val, 5, content) for content in range(3)]
    oracles = [_row_oracle(n_val, 5, content, k) for content in range(3)]
    o_train = _row_oracle(n_train, 0, 0, k)
    assert fr.unsaturated_share(o_train) >= 0.8 and min(fr.unsaturated_share(o) for o in oracles) >= 0.8
    ids = np.stack([np.random.default_rng(k + it).permutation(n_train)[:batch].astype(np.int32) for it in range(n_iters)])
    dev = gf.DeviceLog(rt, log, k, max_batch, 0)
    try:
        params = gf.Params(rt, *th)
        val, other = fr.DeviceRows(rt, logs[0]), fr.DeviceRows(rt, logs[2])
        assert dev.plan.layout()["row_blocks"] == (0 if expect.get("ride_val") is not None else 1)

        def run(rows, content, register):
            if register:
                ph.register_log(dev, 0, rows)
                ph.register_log(dev, 1, rows)
            forms = fr.train_forms(rt, dev.plan, batch, n_iters, 0, rows, n_val)
            tl, vl = fr.train_lr0(rt, dev, params, ids, rows)
            scores = ph.plan_forward(dev, rows, params)
            want, tol = fr.loss_oracle(oracles[content], k, logs[content]["labels"], logs[content]["pscores"])
            for it in range(n_iters):
                fr.assert_loss(vl[it], want, tol, f"{name}: contents {content}, validation loss of iteration {it}")
                w, t = fr.loss_oracle(o_train.take(ids[it]), k, log["labels"][ids[it]], log["pscores"][ids[it]])
                fr.assert_loss(tl[it], w, t, f"{name}: contents {content}, train loss of iteration {it}")
            fr.assert_scores(scores, oracles[content], k, f"{name}: contents {content}")
            return forms, tl, vl, scores

        a = run(val, 0, True)
        assert all(a[0][key] == v for key, v in expect.items()), a[0]
        _overwrite(val, logs[1])
        b = run(val, 1, True)
        assert b[0] == a[0] and not np.array_equal(a[2], b[2]) and not np.array_equal(a[3], b[3])
        again = run(val, 1, False)
        assert again[0] == b[0]
        c = run(other, 2, False)
        assert c[0]["ride_val"] == 0  # (not the registered arrays)
        last = run(val, 1, False)
        for label, r in (("the same arrays", again), ("the same arrays after others", last)):
            assert r[0] == b[0], (label, r[0], b[0])  # (the forms: the validation rows ride again where they did)
            for x, y, what in zip(b[1:], r[1:], ("train losses", "validation losses", "scores")):
                _same(x, y, f"{name}: {what} of {label} without registering again")
    finally:
        dev.close()


# --------------------------------------------------------------------------
# 5. the comparison sees one row
# --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["k32-lanes8", "k65-chunked"])
def test_one_other_row_changes_the_bits_of_the_sparse_class(rt, name):
    """The reference call with ONE row id replaced by another row that is not empty: History.compare
    must fail on the sparse class, and the two dense gradients differ there (a helper that compared a
    buffer with itself would pass both)."""
    h = History(rt, name)
    try:
        h.assert_kind()
        X = h.log["features"]
        sparse = np.flatnonzero(np.diff(X.indptr) > 0)
        sparse = sparse[X.indices[X.indptr[sparse + 1] - 1] >= ph.N_FREQ]  # rows whose last column is a sparse one
        ids = ph.next_ids(np.random.default_rng(3), h.n_rows, h.sizes["min+1"], "fresh", None)
        swapped = ids.copy()
        swapped[np.flatnonzero(np.isin(ids, sparse))[-1]] = np.setdiff1d(sparse, ids)[0]
        assert (swapped != ids).sum() == 1 and len(np.unique(swapped)) == len(ids)
        c = ph.Call("grad", "min+1", "fresh")
        theta0, G0 = h.params.host(), h.accs.host()
        got = h.execute(h.dev, c, ids, h.params, h.accs)
        fresh = h.open()
        try:
            want = h.execute(fresh, c, swapped, gf.Params(rt, *theta0), gf.Params(rt, *G0), SGD)
            same = h.execute(fresh, c, ids, gf.Params(rt, *theta0), gf.Params(rt, *G0), SGD)
        finally:
            fresh.close()
        h.compare("the same ids", c, ids, got, same, theta0, G0)
        with pytest.raises(AssertionError):
            h.compare("one other row", c, ids, got, want, theta0, G0)
        cold = np.setdiff1d(np.arange(ph.N_COLS), h.hot_cols)
        V1, w1, _ = gf.split_grad(got["grad"], ph.N_COLS, h.k)
        V2, w2, _ = gf.split_grad(want["grad"], ph.N_COLS, h.k)
        assert not np.array_equal(_bits(V1[cold]), _bits(V2[cold])) and not np.array_equal(_bits(w1[cold]), _bits(w2[cold]))
    finally:
        h.close()
