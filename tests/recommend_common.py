"""Shared by the catalogue-scoring tests (test_recommend_host.py, test_gpu_recommend.py) and the
generator of their fixture (golden/make_golden_recommend.py): the side matrices of the two
layouts built on the host with SciPy, and the NumPy statement of the identity

    logit(u,i) = w0 + L(xu) + L(xi) + a_u . b_i

(DESIGN.md 8 N5).  Nothing here touches the GPU or the package under test."""
import numpy as np
from scipy import sparse as sp

from oracle import cpu_ref

LAYOUTS = ("kuairec", "coat")
FM_CASES = ((16, 0.25), (16, 2.0), (33, 0.25), (33, 2.0), (400, 0.25), (400, 2.0))  # (k, alpha)
MF_FACTORS = (24, 33)
N_USERS, N_ITEMS = 61, 203


def make_tables(rng, nu=N_USERS, ni=N_ITEMS):
    """User table (30 0/1 columns, density 0.25), item table (4 normal + 31 tag columns of
    density 0.1), one normal context value per user -- dense arrays."""
    user = (rng.random((nu, 30)) < 0.25).astype(np.float64)
    item = np.hstack([rng.standard_normal((ni, 4)), (rng.random((ni, 31)) < 0.1).astype(np.float64)])
    ctx = rng.standard_normal((nu, 1))
    return user, item, ctx


def side_matrices(layout, user, item, ctx):
    """``(XU [nu, F], XI [ni, F])``: pair row (u, i) of the layout is ``XU[u] + XI[i]``."""
    ut, it, cx = sp.csr_matrix(user), sp.csr_matrix(item), sp.csr_matrix(ctx)
    nu, ni = ut.shape[0], it.shape[0]
    U, I = sp.identity(nu, format="csr"), sp.identity(ni, format="csr")
    z = lambda n, w: sp.csr_matrix((n, w))  # noqa: E731
    if layout == "kuairec":   # [one-hot user | one-hot item | context | user table | item table]
        XU = sp.hstack([U, z(nu, ni), cx, ut, z(nu, it.shape[1])])
        XI = sp.hstack([z(ni, nu), I, z(ni, 1), z(ni, ut.shape[1]), it])
    elif layout == "coat":    # [one-hot user | user table | one-hot item | item table]
        XU = sp.hstack([U, ut, z(nu, ni), z(nu, it.shape[1])])
        XI = sp.hstack([z(ni, nu), z(ni, ut.shape[1]), I, it])
    else:
        raise ValueError(layout)
    XU, XI = XU.tocsr(), XI.tocsr()
    XU.sort_indices()
    XI.sort_indices()
    return XU, XI


def pair_rows(XU, XI, users, items):
    X = (XU[np.asarray(users)] + XI[np.asarray(items)]).tocsr()
    X.sort_indices()
    return X


def all_pairs(nu, ni):
    return np.repeat(np.arange(nu), ni), np.tile(np.arange(ni), nu)


def fm_logits(XU, XI, w0, w, V):
    def side(S):
        a = S.dot(V)
        lin = np.asarray(S.dot(w)).ravel()
        return a, lin + 0.5 * ((a ** 2).sum(axis=1) - np.asarray(S.power(2).dot(V ** 2)).sum(axis=1))

    a, LU = side(XU)
    b, LI = side(XI)
    return float(np.ravel(w0)[0]) + LU[:, None] + LI[None, :] + a @ b.T


def mf_logits(P, Q, b_u, b_i, b):
    return float(b) + b_u[:, None] + b_i[None, :] + P @ Q.T


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-np.clip(z, -700, 700)))  # src/base.py:63-66


def stable_topk(logit_row, k):
    """``np.argsort(logit, kind="stable")[::-1]`` with the NaNs removed, first k."""
    order = np.argsort(logit_row, kind="stable")[::-1]
    return order[~np.isnan(logit_row[order])][:k]


def case_name(k, alpha):
    """Key prefix of an FM case in ``recommend_fm_<layout>.npz``."""
    return f"k{k}_a{int(round(alpha * 100)):03d}"


def fm_parameters(g, gl, layout, k, alpha, tight=1e-9):
    """``w0, w, V`` of a fixture case (``g``: recommend.npz, ``gl``: the layout's file); for k = 400,
    whose V is not stored, refitted by the oracle from the stored log."""
    name = case_name(k, alpha)
    if f"{name}_V" in gl.files:
        return gl[f"{name}_w0"], gl[f"{name}_w"], gl[f"{name}_V"]
    XU, XI = side_matrices(layout, g["user_table"], g["item_table"], g["context"])
    X = pair_rows(XU, XI, g["log_users"], g["log_items"])
    n = int(g["n_log"])
    train = {"features": X[:n], "labels": g["labels"][:n], "pscores": g["pscores"][:n]}
    fit = cpu_ref.fm_fit(train, None, n_epochs=int(g["fm_iters"]), n_factors=k, lr=float(gl[f"{name}_lr"]),
                         batch_size=int(g["batch_size"]), seed=int(g["seed"]), alpha=alpha, with_losses=False)
    # the refit is the reference's fit: its w and w0 (stored for every case) say so
    for got, want in ((fit["w"], gl[f"{name}_w"]), (fit["w0"], gl[f"{name}_w0"])):
        assert np.max(np.abs(got - want)) <= tight * np.max(np.abs(want)), name
    return fit["w0"], fit["w"], fit["V"]
