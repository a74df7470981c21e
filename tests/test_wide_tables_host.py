"""The harness of test_gpu_wide_tables.py cannot hide the defect it looks for (no GPU needed).

wide_tables_common.VirtualTable is a NumPy model of a wide table -- its live rows, NaN elsewhere --
with a gather and a scatter whose row offsets are formed correctly, reduced to 32 bits of bytes, or
masked to 31 bits of element index.  For EVERY id map the GPU cases use, a kernel that wraps must be
seen: the comparison of the live rows (a) or the census (b) fails for each wrapped variant of each
threshold the map's table crosses, and both pass for the correct kernel.  A live-id set for which a
wrapped model passes is a broken case; the last test shows one (every id below the threshold) so
that the assertion over the real maps is known to be able to fail."""
import numpy as np
import pytest

import mf_step_common as ms
import wide_tables_common as wt


def _step_maps():
    """The maps test_gpu_wide_tables.py makes for the MF step cases: one per side of each case."""
    out = {}
    for name in wt.MF_STEP_CASES:
        case = wt.mf_step_case(name)
        for side, count in (("P", case.n_users), ("Q", case.n_items)):
            out[f"mf-{side}-{name}"] = wt.step_map(name, count)
    return out


def _all_maps():
    maps = {name: wt.id_map(name) for name in wt.MAPS}
    maps.update(_step_maps())
    return maps


ALL_MAPS = _all_maps()


@pytest.mark.parametrize("name", sorted(ALL_MAPS))
def test_every_map_has_the_live_ids_the_method_names(name):
    imap = ALL_MAPS[name]
    imap.assert_sizes()
    live = set(imap.wide.tolist())
    assert {0, 1, 2} <= live and imap.n - 1 in live
    for kind, t in imap.T.items():
        assert {t - 1, t, t + 1} <= live
        # the table is JUST past the threshold: a margin of a few rows
        assert imap.n - t <= wt.MARGIN + (imap.top - t)
    assert imap.n <= 17_000_000   # no case needs more rows than the 8-lane forward's k = 32


@pytest.mark.parametrize("name", sorted(ALL_MAPS))
def test_a_wrapped_offset_fails_on_every_map(name):
    imap = ALL_MAPS[name]
    assert wt.model_verdicts(imap.wide, imap.n, imap.width, None) == (True, True)
    for kind in imap.kinds:
        gather_ok, scatter_ok = wt.model_verdicts(imap.wide, imap.n, imap.width, kind)
        assert not gather_ok, f"{name}: a gather that wraps at {kind} reads the compact rows"
        assert not scatter_ok, f"{name}: a scatter that wraps at {kind} passes the comparison and the census"


@pytest.mark.parametrize("name", sorted(ALL_MAPS))
def test_the_wrapped_row_is_a_guard_row_or_a_live_row_of_other_contents(name):
    """Where the wrapped access of each live id at or above T lands: on a live row (other contents:
    the comparison fails) or on a guard row (NaN: the comparison and the census fail) -- never on
    the row itself."""
    imap = ALL_MAPS[name]
    for kind, t in imap.T.items():
        high = imap.wide[imap.wide >= t]
        assert len(high) >= 3
        e = wt.element_offsets(high, imap.width, kind)
        assert (e != wt.element_offsets(high, imap.width)).all() and e.max() < imap.n * imap.width
        rows = np.unique(e // imap.width)
        assert not set(rows.tolist()) & set(high.tolist())


@pytest.mark.parametrize("kind", [wt.T32B, wt.T31E])
def test_ids_below_the_threshold_hide_the_defect(kind):
    """The broken case: the same table, every live id below T.  The wrapped model passes, so the
    assertions above hold because of the ids the maps choose."""
    imap = wt.IdMap(wt.FM_COLS, 128, (kind,))
    low = np.arange(wt.FM_COLS)
    assert low.max() < imap.T[kind]
    assert wt.model_verdicts(low, imap.n, imap.width, kind) == (True, True)


def test_the_dense_gradient_regions_lie_past_the_threshold():
    """rfm_fm_grad's buffer is [G_V (n k) | g_w (n) | g_w0]: with n k past 2^29 every element of g_w
    and g_w0 has an offset past T32b, whatever its column."""
    imap = wt.id_map("fm-V-k128")
    assert imap.n * imap.width >= 1 << 29
    assert ((imap.n * imap.width + imap.wide) * 8 >= 2 ** 32).all()


def test_step_cases_are_the_builders_of_mf_step_common():
    for name, (k, kinds) in wt.MF_STEP_CASES.items():
        case = wt.mf_step_case(name)
        cls = ms.shape_class(k)
        assert case.k == k and cls == ((64, 2, 1) if k == 128 else (64, 2, 8))
        assert ms.CLASS_RANGE[cls][1] == k   # the largest factor count of its class: the fewest rows
        assert case.want_plan["levels_ex"][0][0] == "wide" and case.want_plan["levels_ex"][1][0] == "seq"


def test_the_gpu_module_takes_every_map_from_the_registry():
    """test_gpu_wide_tables.py makes no id map of its own: every one comes from wt.id_map (a name of
    wt.MAPS) or wt.step_map (a name of wt.MF_STEP_CASES), both of which refuse a name that is not
    registered, and every registered name is used there -- so ALL_MAPS above is the set the GPU cases
    run on."""
    import os
    import re
    src = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "test_gpu_wide_tables.py")).read()
    assert "IdMap(" not in src
    with pytest.raises(KeyError):
        wt.id_map("not-registered")
    with pytest.raises(KeyError):
        wt.step_map("not-registered", 40)
    literal = set(re.findall(r'"([a-zA-Z0-9-]+)"', src))
    patterns = {f"fm-V-k{k}" for k in (32, 128, 1024)} | {f"mf-{s}-predict-k128" for s in "PQ"}
    assert 'f"fm-V-k{k}"' in src and 'f"mf-{side}-predict-k{k}"' in src
    unused = set(wt.MAPS) - literal - patterns
    assert not unused, unused
    assert set(wt.MF_STEP_CASES) <= literal


def test_the_wide_output_case_wraps_onto_another_pair():
    """test_pair_scores_wide_output has no id map: its table is the OUTPUT, whose rows are the selected
    users.  The same model: a store at ``s * n_items + item`` reduced to 32 bits of bytes lands, for
    every user from T on, on an element of a user below T -- whose own score then differs from the
    call on the item sub-ranges -- and leaves its own element NaN, which the census counts."""
    n_items, n_sel = wt.WIDE_OUT_ITEMS, wt.WIDE_OUT_SEL
    t = wt.threshold_row(wt.T32B, n_items)
    assert n_sel == t + wt.MARGIN == 133 and n_sel * n_items * 8 > 2 ** 32 > t * n_items * 8 - n_items * 8
    s = np.arange(t, n_sel, dtype=np.int64)
    for item in (0, 1, n_items // 2, n_items - 1):
        e = s * n_items + item
        assert (e >= 1 << 29).all()
        wrapped = e & wt.MASK_T32B
        assert (wrapped // n_items < t).all() and (wrapped != e).all()
