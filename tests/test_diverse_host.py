"""Host half of the diversified re-ranking tests (no GPU): the float64 statement of
diverse_common.py against its long-double oracle on every case list, the condition on the inputs --
every step of every list of every random case list is separated, share 1.0 --, the floor under the
derived tolerances, an independent plain NumPy MMR, six mutations of the statement each refused by
the checkers the GPU tests go through (and on the affected lists alone), the header's new entries
against the ctypes table, the geometry of every GPU case list, and the argument checks of
recommend.py that need no device."""
import inspect
import os
import re

import numpy as np
import pytest

import diverse_common as dc
import pair_tile_common as pc
from diverse_common import LD, U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST_LISTS, HOST_K = 4, 64
HOST_CASES = [(kf, depth) for kf in dc.HOST_FACTORS for depth in dc.HOST_DEPTHS]


def _similarities_floor(c, o, what):
    """Every similarity the statement forms for the oracle's picks, factors as stored and shuffled, within
    half of (c + 7) u S of the long-double dot product."""
    kf = c.kf
    D = LD(-(-kf // dc.LANES) + 7) * LD(U) * LD(dc.SECOND_ORDER)
    shuffle = np.random.default_rng(kf).permutation(kf)
    Rl, Ra = c.R.astype(LD), np.abs(c.R).astype(LD)
    worst = 0.0
    for l in range(c.n_lists):
        C = c.R[c.items[l]]
        for j in np.unique(o.items[l][o.items[l] >= 0]):
            want, S = Rl[c.items[l]] @ Rl[j], Ra[c.items[l]] @ Ra[j]
            for cols in (np.arange(kf), shuffle):
                got = dc.sims_statement(C[:, cols], c.R[j][cols], kf)
                worst = max(worst, float(pc.excess(got, want, D * S).max()))
    print(f"{what}: largest |d sim| / tol {worst:.3g}")
    assert worst <= 0.5, (what, worst)


@pytest.mark.parametrize("kf,depth", HOST_CASES)
def test_statement_against_the_oracle_and_the_floor(kf, depth):
    """The statement makes the oracle's picks with values inside the tolerance -- on the issue's case lists
    (no penalty) inside HALF of it, with the factors as stored and shuffled -- and every step of every
    list is separated."""
    c = dc.case(HOST_LISTS, depth, kf)
    shuffle = np.random.default_rng(kf + depth).permutation(kf)
    for lam in dc.HOST_LAMBDAS:
        for penalty in ((None, c.penalty) if depth == 65 else (None,)):  # (the issue's cases, and a penalty at one depth)
            what = f"factors={kf} depth={depth} lambda={lam} penalty={penalty is not None}"
            o = dc.select_oracle(c.items, c.scores, c.R, kf, penalty, lam, HOST_K)
            print(f"{what}: separated share {o.separated.mean():.4f}, smallest margin {o.gap:.3g}, "
                  f"largest tolerance {float(o.tol.max()):.3g}")
            assert o.separated.all() and (o.pos >= 0).all(), what
            for name, cols in (("natural", np.arange(kf)), ("shuffled", shuffle)):
                got = dc.select_statement(c.items, c.scores, c.R[:, cols], kf, penalty, lam, HOST_K)
                # with a penalty step 0 is two roundings of numbers just above 1/4, each of which may come
                # as close to its u |x| as it likes: no floor below the tolerance follows, the tolerance holds
                dc.assert_against_oracle(got, o, c.scores, f"{what} {name}", bound=0.5 if penalty is None else 1.0)
    _similarities_floor(c, o, f"factors={kf} depth={depth}")


@pytest.mark.parametrize("name,shape,k", dc.random_gpu_cases(), ids=[n for n, _, _ in dc.random_gpu_cases()])
def test_gpu_case_lists_are_separated_and_have_the_geometry_they_name(name, shape, k):
    c = dc.case(*shape)
    for lam in (0.3, 0.7):
        for penalty in (None, c.penalty):
            o = dc.select_oracle(c.items, c.scores, c.R, c.kf, penalty, lam, k)
            assert o.separated.all(), (name, lam, penalty is not None, o.gap)
            assert ((o.pos >= 0).sum(axis=1) == min(k, c.depth)).all()
    g = dc.geometry(c.n_lists, c.depth, c.kf, k=k)
    assert g == dict(form=0, workgroups=c.n_lists, passes=1, candidates_per_thread=-(-c.depth // dc.BLOCK),
                     lds_bytes=(2 * dc.MAX_DEPTH + 1024) * 8 + dc.MAX_DEPTH * 4 + 64, factor_trips=-(-c.kf // dc.LANES)), g


def test_geometry_of_the_grid_and_its_refusals():
    from relevance_factorizationmachine_amd import _lib
    cap = dc.geometry(10 ** 6, 5, 5)["workgroups"]
    assert cap == 256 * 5 and cap * dc.geometry(1, 5, 5)["lds_bytes"] // 256 <= 160 << 10
    assert dc.geometry(cap, 5, 5)["passes"] == 1
    g = dc.geometry(cap + 1, 5, 5)
    assert (g["workgroups"], g["passes"]) == (cap, 2)  # the smallest count that gives a workgroup its second list
    assert dc.geometry(0, 5, 5)["workgroups"] == 0
    assert dc.geometry(3, 1024, 1024, ld_R=1024, k=64)["candidates_per_thread"] == 4
    for bad in (dict(depth=0), dict(depth=1025), dict(kf=0), dict(kf=1025), dict(k=0), dict(k=65), dict(kf=5, ld_R=4),
                dict(n_lists=-1)):
        args = dict(n_lists=3, depth=65, kf=5, ld_R=None, k=9)
        args.update(bad)
        with pytest.raises(ValueError):
            dc.geometry(**args)
    assert _lib.RFM_ERR_BAD_ARG == 1


@pytest.mark.parametrize("kf", dc.HOST_FACTORS)
def test_plain_numpy_mmr_agrees_on_the_separated_cases(kf):
    for depth in (65, 257):
        c = dc.case(HOST_LISTS, depth, kf)
        for lam in dc.HOST_LAMBDAS:
            for penalty in (None, c.penalty):
                o = dc.select_oracle(c.items, c.scores, c.R, kf, penalty, lam, 16)
                items, pos = dc.plain_mmr(c.items, c.scores, c.R, kf, penalty, lam, 16)
                assert o.separated.all() and (items == o.items).all() and (pos == o.pos).all(), (kf, depth, lam)


def test_trade_off_one_returns_the_first_eligible_candidates_in_order():
    c = dc.case(3, 65, 37)
    items, scores, values, pos = dc.select_statement(c.items, c.scores, c.R, 37, None, 1.0, 9)
    assert (pos == np.arange(9)[None, :]).all() and (items == c.items[:, :9]).all()
    assert values.tobytes() == c.scores[:, :9].tobytes() == scores.tobytes()
    s = dc.special_case()
    R = s.R.copy()
    R[71] = 1.0  # (an infinite similarity times 1 - lambda = 0 is a NaN value: that case is the special inputs' own)
    items, scores, values, pos = dc.select_statement(s.items, s.scores, R, s.kf, None, 1.0, 64)
    eligible = [p for p in range(s.depth) if 0 <= s.items[0, p] < s.n_items and not np.isnan(s.scores[0, p])]
    # (the repeat at position 9 has position 5's score: it follows it at once, the lower position first)
    want = sorted(eligible, key=lambda p: (-s.scores[0, p], -s.items[0, p], p))
    assert pos[0, :len(want)].tolist() == want and (pos[0, len(want):] == -1).all()
    assert want[:5] == eligible[:5] and want.index(9) == want.index(5) + 1
    assert (items[0, len(want):] == -1).all() and np.isnan(scores[0, len(want):]).all() and np.isnan(values[0, len(want):]).all()


def test_statement_on_the_special_inputs():
    s = dc.special_case()
    w = s.where
    for lam in (0.3, 0.7):
        for penalty in (None, s.penalty):
            items, scores, values, pos = dc.select_statement(s.items, s.scores, s.R, s.kf, penalty, lam, 64)
            chosen = pos[0][pos[0] >= 0]
            n_eligible = s.depth - len(w["outside"]) - 1 - len(w["padded"])
            assert len(chosen) == n_eligible == len(set(chosen.tolist())), "every eligible candidate once, nothing else"
            assert not set(chosen.tolist()) & (set(w["outside"]) | {w["nan_score"]} | set(w["padded"]))
            assert ((items[0] >= 0) == (pos[0] >= 0)).all() and items[0].max() < s.n_items
            assert {w["nan_row"], w["inf_row"]} <= set(chosen.tolist()), "rows without a direction are candidates still"
            assert list(chosen).index(w["repeat"][0]) < list(chosen).index(w["repeat"][1])
            if penalty is None:
                assert pos[0, 0] == w["nan_row"], "the highest score goes first"
                # nothing is similar to a row without a direction: the second pick is by relevance alone
                assert values[0, 1] == np.float64(lam) * s.scores[0, pos[0, 1]] - (np.float64(1.0) - np.float64(lam)) * 0.0


def test_statement_on_the_planted_twins():
    tw = dc.twin_case()
    lo, hi = tw.twins
    items, scores, values, pos = dc.select_statement(tw.items, tw.scores, tw.R, tw.kf, None, 1.0, 9)
    assert (items[:, 0] == hi).all() and (items[:, 1] == lo).all(), "adjacent picks, the higher id first"
    assert values[:, 0].tobytes() == values[:, 1].tobytes() and scores[:, 0].tobytes() == scores[:, 1].tobytes()
    items, _, values, _ = dc.select_statement(tw.items, tw.scores, tw.R, tw.kf, tw.penalty * 0, 0.5, 9)
    assert (items[:, 0] == hi).all(), "an exact tie goes to the higher id"
    o = dc.select_oracle(tw.items, tw.scores, tw.R, tw.kf, None, 0.5, 9)
    assert not o.separated[:, 0].any(), "the oracle knows the tie for what it is"


# --------------------------------------------------------------------------
# mutations
# --------------------------------------------------------------------------
def _oracle_refuses_only(c, R, items, penalty, lam, k, mutation, affected):
    """The oracle checker accepts the statement on every list, accepts the mutated statement on the lists
    outside ``affected`` and refuses it on each list of ``affected`` by itself."""
    o = dc.select_oracle(items, c.scores, R, c.kf, penalty, lam, k)
    assert o.separated.all()
    dc.assert_against_oracle(dc.select_statement(items, c.scores, R, c.kf, penalty, lam, k), o, c.scores, "statement")
    bad = dc.select_statement(items, c.scores, R, c.kf, penalty, lam, k, mutation)
    others = [l for l in range(c.n_lists) if l not in affected]
    dc.assert_against_oracle(bad, o, c.scores, f"{mutation}: unaffected lists", others)
    for l in affected:
        assert dc.refuses(dc.assert_against_oracle, bad, o, c.scores, f"{mutation}: list {l}", [l]), (mutation, l)


def _identity(c, penalty, lam, k, mutation):
    a = dc.select_statement(c.items, c.scores, c.R, c.kf, penalty, lam, k)
    b = dc.select_statement(c.items, c.scores, c.R, c.kf, penalty, lam, k, mutation)
    dc.assert_same_bits(b, a, f"{mutation} where it changes nothing")


@pytest.mark.parametrize("lam", dc.HOST_LAMBDAS)
def test_mutation_mean_instead_of_maximum(lam):
    c = dc.case(4, 65, 5)
    _oracle_refuses_only(c, c.R, c.items, c.penalty, lam, 9, "mean_similarity", range(4))
    _identity(c, c.penalty, lam, 2, "mean_similarity")  # (one pick: its mean is its maximum)


@pytest.mark.parametrize("lam", dc.HOST_LAMBDAS)
def test_mutation_maximum_without_the_most_recent_pick(lam):
    c = dc.case(4, 65, 5)
    _oracle_refuses_only(c, c.R, c.items, None, lam, 9, "stale_maximum", range(4))
    _identity(c, None, lam, 1, "stale_maximum")


def test_mutation_ties_to_the_lower_id():
    tw = dc.twin_case()
    for lam in (1.0, 0.5):
        good = dc.select_statement(tw.items, tw.scores, tw.R, tw.kf, None, lam, 9)
        bad = dc.select_statement(tw.items, tw.scores, tw.R, tw.kf, None, lam, 9, "ties_to_lower_id")
        for l in range(tw.n_lists):
            assert dc.refuses(dc.assert_same_bits, bad, good, f"twins list {l}", [l])
    _identity(dc.case(4, 65, 5), None, 0.5, 9, "ties_to_lower_id")  # (no tie: nothing to decide)


def test_mutation_nan_similarity_makes_a_candidate_ineligible():
    c = dc.case(4, 65, 5)
    R = np.vstack([c.R, np.full((1, c.kf), np.nan)])
    items = c.items.copy()
    items[:2, 0] = c.n_items  # lists 0 and 1: the most relevant candidate has no direction
    _oracle_refuses_only(c, R, items, None, 0.7, 9, "nan_similarity_ineligible", (0, 1))


def test_mutation_penalty_added():
    c = dc.case(4, 65, 5)
    R = np.vstack([c.R, dc.case(1, 65, 5, 9).R[:1]])
    items = c.items.copy()
    items[:2, 0] = c.n_items  # the one item with a penalty, a candidate of lists 0 and 1 alone
    penalty = np.zeros(c.n_items + 1)
    penalty[c.n_items] = 0.15
    _oracle_refuses_only(c, R, items, penalty, 0.7, 9, "penalty_added", (0, 1))


@pytest.mark.parametrize("kf", (1, 65, 129))
def test_mutation_dot_product_drops_the_last_factor(kf):
    c = dc.case(4, 65, kf)
    _oracle_refuses_only(c, c.R, c.items, None, 0.3, 9, "drops_last_factor", range(4))
    for other in (5, 64, 66):  # at any other n_factors % 64 the mutation is the statement itself
        _identity(dc.case(4, 65, other), None, 0.3, 9, "drops_last_factor")


# --------------------------------------------------------------------------
# the ABI table and the Python checks that need no device
# --------------------------------------------------------------------------
def test_header_declares_the_new_entries_as_the_ctypes_table_has_them():
    """include/rfm_diverse.h (which rfm_hip.h includes where the catalogue entries stand) against
    ``_lib.DIVERSE_SIGNATURES``, argument by argument; the library exports both and binds them."""
    import ctypes as C

    from relevance_factorizationmachine_amd import _lib
    main = open(os.path.join(ROOT, "include", "rfm_hip.h")).read()
    header = open(os.path.join(ROOT, "include", "rfm_diverse.h")).read()
    assert main.count('#include "rfm_diverse.h"') == 1 and main.index('#include "rfm_diverse.h"') > main.index("rfm_pair_order_geometry")
    declarations = r"^int32_t\s+(rfm_\w+)\s*\(([^)]*)\)\s*;"
    found = re.findall(declarations, re.sub(r"/\*.*?\*/", " ", header, flags=re.S), flags=re.M)
    assert [name for name, _ in found] == list(_lib.DIVERSE_SIGNATURES) == ["rfm_diverse_select", "rfm_diverse_geometry"]
    assert not set(_lib.DIVERSE_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.NEIGHBOUR_SIGNATURES) | set(_lib.AUDIENCE_SIGNATURES))
    kinds = {C.c_int32: "int32_t", C.c_int64: "int64_t", C.c_double: "double"}
    lib = _lib.load()
    for name, params in found:
        params = [re.sub(r"\bconst\b", "", p).strip() for p in params.split(",")]
        want = ["pointer" if "*" in p else p.split()[0] for p in params]
        got = [kinds.get(t, "pointer") for t in _lib.DIVERSE_SIGNATURES[name]]
        assert want == got, (name, want, got)
        assert getattr(lib, name).argtypes == _lib.DIVERSE_SIGNATURES[name] and getattr(lib, name).restype is C.c_int32
    assert "rfm_diverse.hip" in _lib.SOURCES and any(h.endswith("rfm_diverse.h") for h in _lib.HEADERS)
    text = re.sub(r"\s*\n \*\s*", " ", header)
    assert "utils/metrics.py:110-166" in text and "no counterpart" in text
    assert "nothing is contracted into an fma" in text and "value descending, then item id descending" in text


def test_check_diverse_defaults_and_refusals():
    from relevance_factorizationmachine_amd import recommend as rec
    assert rec.check_diverse(10728, 9) == (9, 64, 0.5, None)
    assert rec.check_diverse(10728, 64)[1] == 256 and rec.check_diverse(40, 9)[1] == 40
    assert rec.check_diverse(203, 9, depth=10 ** 6)[1] == 203  # (clamped: the full ordering)
    assert rec.check_diverse(5000, 9, depth=1024)[1] == 1024
    k, depth, lam, pen = rec.check_diverse(7, 2, 5, 1, "dot", [0, 1, 2, 3, 4, 5, 6])
    assert (k, depth, lam) == (2, 5, 1.0) and pen.dtype == np.float64 and pen.tolist() == [0, 1, 2, 3, 4, 5, 6]
    for k in (0, 65, -1, 2.5, True):
        with pytest.raises(ValueError, match="outside 1..64"):
            rec.check_diverse(100, k)
    with pytest.raises(ValueError, match="at most 1024 candidates"):
        rec.check_diverse(5000, 9, depth=1025)
    with pytest.raises(ValueError, match="at most 1024 candidates"):
        rec.check_diverse(5000, 9, depth=10 ** 6)
    with pytest.raises(ValueError, match="depth must be an integer"):
        rec.check_diverse(100, 9, depth=64.0)
    with pytest.raises(ValueError, match="at least 1"):
        rec.check_diverse(100, 9, depth=0)
    with pytest.raises(ValueError, match="k=9 picks from depth=8 candidates"):
        rec.check_diverse(100, 9, depth=8)
    with pytest.raises(ValueError, match="k=9 picks from depth=5 candidates"):
        rec.check_diverse(5, 9)
    for lam in (-0.1, 1.0000001, float("nan"), float("inf")):
        with pytest.raises(ValueError, match=r"outside \[0, 1\]"):
            rec.check_diverse(100, 9, trade_off=lam)
    with pytest.raises(ValueError, match="trade_off must be a number"):
        rec.check_diverse(100, 9, trade_off="half")
    with pytest.raises(ValueError, match="neither 'cosine' nor 'dot'"):
        rec.check_diverse(100, 9, metric="jaccard")
    with pytest.raises(ValueError, match=r"item_penalty has shape \(99,\), expected \(100,\)"):
        rec.check_diverse(100, 9, item_penalty=np.zeros(99))
    with pytest.raises(ValueError, match="item_penalty has shape"):
        rec.check_diverse(100, 9, item_penalty=np.zeros((100, 1)))
    bad = np.zeros(100)
    bad[17] = np.nan
    with pytest.raises(ValueError, match="item_penalty holds a NaN"):
        rec.check_diverse(100, 9, item_penalty=bad)


def test_model_methods_exist_with_the_issue_s_signatures():
    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import recommend as rec
    tail = ["k", "depth", "trade_off", "users", "exclude", "metric", "item_penalty", "new_users"]
    for cls, lead in ((pkg.LogisticMatrixFactorization, ["self"]), (pkg.FactorizationMachines, ["self", "sides"])):
        sig = inspect.signature(cls.recommend_diverse)
        assert list(sig.parameters) == lead + tail
        assert [sig.parameters[n].default for n in tail[1:]] == [None, 0.5, None, None, "cosine", None, None]
    assert list(inspect.signature(rec.diverse).parameters) == ["model", "sides"] + tail
    assert list(inspect.signature(rec.diversify).parameters) == ["rt", "cand_items", "cand_scores", "R", "n_factors", "k",
                                                                 "trade_off", "item_penalty"]
    names = list(inspect.signature(rec.rank_catalogue_device).parameters)
    assert names == list(inspect.signature(rec.rank_catalogue).parameters)
