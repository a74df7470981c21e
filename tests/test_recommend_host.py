"""Catalogue scoring and top-K, the part that needs no GPU: argument checks of ``recommend.Sides``
and of the top-K size, and the identity

    logit(u,i) = w0 + L(xu) + L(xi) + a_u . b_i

pinned to the REFERENCE's ``predict()`` over the materialised rows of all pairs
(``tests/golden/recommend*.npz``, written by ``make_golden_recommend.py``).  Tolerances are those of
``tests/test_gpu_parity.py``, unchanged."""
import numpy as np
import pytest
from scipy import sparse as sp

import recommend_common as rc
from conftest import assert_elementwise, load_golden, rel_err
from oracle import cpu_ref

CONTRACT = 1e-5
TIGHT = 1e-9


_case, fm_parameters = rc.case_name, rc.fm_parameters


def test_sides_reject_overlap_and_widths():
    from relevance_factorizationmachine_amd import recommend

    XU = sp.csr_matrix(np.array([[1.0, 0, 0, 2.0, 0], [0, 1.0, 0, 0, 0]]))
    XI = sp.csr_matrix(np.array([[0, 0, 1.0, 0, 0], [0, 0, 0, 0, 3.0], [0, 0, 1.0, 0, 1.0]]))
    s = recommend.Sides(user_rows=XU, item_rows=XI)
    assert (s.n_users, s.n_items, s.n_features) == (2, 3, 5)
    clash = XI.copy().tolil()
    clash[1, 3] = 7.0
    with pytest.raises(ValueError, match="column 3"):
        recommend.Sides(user_rows=XU, item_rows=clash.tocsr())
    # a stored zero on both sides is a stored column on both sides
    stored_zero = sp.csr_matrix((np.array([0.0]), np.array([0]), np.array([0, 1, 1, 1])), shape=(3, 5))
    with pytest.raises(ValueError, match="column 0"):
        recommend.Sides(user_rows=XU, item_rows=stored_zero)
    with pytest.raises(ValueError, match="same width"):
        recommend.Sides(user_rows=XU, item_rows=sp.csr_matrix((3, 6)))
    with pytest.raises(ValueError):
        recommend.Sides(user_rows=XU, item_rows=sp.csr_matrix((0, 5)))


@pytest.mark.parametrize("k", [0, -1, 65, 1000])
def test_topk_size_outside_1_to_64_is_rejected(k):
    from relevance_factorizationmachine_amd import recommend

    with pytest.raises(ValueError, match="outside 1..64"):
        recommend.topk_workspace_bytes(61, 203, k)


def test_topk_workspace_grows_with_k_and_users():
    from relevance_factorizationmachine_amd import recommend

    assert recommend.MAX_K == 64
    a, b, c = (recommend.topk_workspace_bytes(61, 203, 1), recommend.topk_workspace_bytes(61, 203, 64),
               recommend.topk_workspace_bytes(1411, 3327, 64))
    assert 0 < a < b < c
    assert recommend.pad4(33) == 36 and recommend.pad4(400) == 400 and recommend.pad4(1) == 4


@pytest.mark.parametrize("layout", rc.LAYOUTS)
@pytest.mark.parametrize("k,alpha", rc.FM_CASES)
def test_identity_matches_reference_predict_fm(layout, k, alpha):
    g, gl = load_golden("recommend"), load_golden(f"recommend_fm_{layout}")
    w0, w, V = fm_parameters(g, gl, layout, k, alpha)
    XU, XI = rc.side_matrices(layout, g["user_table"], g["item_table"], g["context"])
    got = rc.sigmoid(rc.fm_logits(XU, XI, w0, w, V))
    R = gl[f"{_case(k, alpha)}_R"]
    assert R.shape == (rc.N_USERS, rc.N_ITEMS)
    print(layout, k, alpha, "rel_err", rel_err(got, R))
    assert rel_err(got, R) < TIGHT
    assert_elementwise(got, R, rtol=CONTRACT, what=f"{layout} {_case(k, alpha)}")


@pytest.mark.parametrize("k", rc.MF_FACTORS)
def test_identity_matches_reference_predict_mf(k):
    g = load_golden("recommend")
    got = rc.sigmoid(rc.mf_logits(g[f"mf_k{k}_P"], g[f"mf_k{k}_Q"], g[f"mf_k{k}_bu"], g[f"mf_k{k}_bi"],
                                  float(g[f"mf_k{k}_b"])))
    assert rel_err(got, g[f"mf_k{k}_R"]) < TIGHT
    assert_elementwise(got, g[f"mf_k{k}_R"], rtol=CONTRACT, what=f"mf k={k}")


def test_side_rows_add_up_to_the_oracle_pair_rows():
    """The host statement of the layouts (recommend_common.side_matrices) against the oracle's
    loaders-in-SciPy, so the fixture's design matrices are the reference layouts."""
    g = load_golden("recommend")
    user, item, ctx = sp.csr_matrix(g["user_table"]), sp.csr_matrix(g["item_table"]), sp.csr_matrix(g["context"])
    uu, ii = rc.all_pairs(rc.N_USERS, rc.N_ITEMS)
    XU, XI = rc.side_matrices("kuairec", g["user_table"], g["item_table"], g["context"])
    want = cpu_ref.fm_features_kuairec(uu, ii, rc.N_USERS, rc.N_ITEMS, ctx[uu], user, item)
    assert abs(rc.pair_rows(XU, XI, uu, ii) - want).nnz == 0
    XU, XI = rc.side_matrices("coat", g["user_table"], g["item_table"], g["context"])
    want = cpu_ref.fm_features_coat(uu, ii, user, item)
    assert abs(rc.pair_rows(XU, XI, uu, ii) - want).nnz == 0
