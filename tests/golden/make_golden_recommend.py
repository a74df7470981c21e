"""Golden vectors for catalogue scoring and top-K, produced by RUNNING THE
REFERENCE (``src/fm.py``, ``src/mf.py``), given the root of its checkout::

    python tests/golden/make_golden_recommend.py REFERENCE_ROOT

61 users x 203 items; a 0/1 user table, an item table of 4 normal + 31 tag columns, one normal
context value per user (``recommend_common.make_tables``); both layouts of the reference's loaders
(``recommend_common.side_matrices``); a 2 000-row log drawn from the pairs.  For every FM case
(k, alpha) the reference model is fitted for 20 iterations (B = 500, IPS, lr = 1e-4 unless the
parameters come out non-finite -- the lr used is stored) and its ``predict()`` over the design
matrix of ALL 12 383 pairs is stored as a [61 x 203] matrix, with w0, w and (k <= 33) V; for
k = 400 the tests refit with ``oracle.cpu_ref.fm_fit`` from the stored log.  MF: k = 24, 33 after 3
iterations (lr = 0.02, reg = 0.5).  Only numeric arrays are stored.  One file would exceed the
repository's 1 MiB limit, so the FM results go to one file per layout:

    recommend.npz              tables, log, MF parameters and matrices
    recommend_fm_kuairec.npz   FM parameters and matrices, KuaiRec layout
    recommend_fm_coat.npz      ... Coat layout
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REF = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else os.environ.get("RFM_REFERENCE_ROOT", "")
sys.path[:0] = [os.path.dirname(HERE), os.path.dirname(os.path.dirname(HERE))]  # tests/ and the repository root

import recommend_common as rc  # noqa: E402

SEED, N_LOG, N_VAL, BATCH, FM_ITERS, MF_ITERS = 12345, 2000, 200, 500, 20, 3
# seed of the tables and the log: chosen so that, on the alpha = 0.25 cases, neighbouring reference
# probabilities inside every user's top 10 are more than 1e-6 apart (printed below; the GPU test
# asserts it before it compares rankings exactly)
TABLE_SEED = 2033


def _import_reference():
    if not os.path.isdir(os.path.join(REF, "src")):
        raise SystemExit("usage: make_golden_recommend.py REFERENCE_ROOT (the reference's checkout)")
    for name in [m for m in sys.modules if m in ("src", "utils") or m.startswith(("src.", "utils."))]:
        del sys.modules[name]
    sys.path.insert(0, REF)
    try:
        from src.fm import FactorizationMachines
        from src.mf import LogisticMatrixFactorization
        import src.fm as _fm
        assert _fm.__file__.startswith(REF), _fm.__file__
    finally:
        sys.path.remove(REF)
    return FactorizationMachines, LogisticMatrixFactorization


def save(name, arrays):
    path = os.path.join(HERE, name + ".npz")
    np.savez_compressed(path, **arrays)
    size = os.path.getsize(path)
    print(f"wrote {path} ({size / 1024:.1f} KiB)")
    assert size < (1 << 20), "fixture over the 1 MiB limit"


def main() -> None:
    FM, MF = _import_reference()
    rng = np.random.default_rng(TABLE_SEED)
    nu, ni = rc.N_USERS, rc.N_ITEMS
    user, item, ctx = rc.make_tables(rng)
    log_users = rng.integers(0, nu, size=N_LOG + N_VAL)
    log_items = rng.integers(0, ni, size=N_LOG + N_VAL)
    labels = (rng.random(N_LOG + N_VAL) < 0.5).astype(np.int64)
    pscores = rng.uniform(0.1, 1.0, size=N_LOG + N_VAL) ** 0.5
    common = dict(user_table=user, item_table=item, context=ctx, log_users=log_users, log_items=log_items,
                  labels=labels, pscores=pscores, n_log=np.int64(N_LOG), seed=np.int64(SEED),
                  batch_size=np.int64(BATCH), fm_iters=np.int64(FM_ITERS), mf_iters=np.int64(MF_ITERS))
    uu, ii = rc.all_pairs(nu, ni)

    def split(features):
        tr = {"features": features[:N_LOG], "labels": labels[:N_LOG], "pscores": pscores[:N_LOG]}
        va = {"features": features[N_LOG:], "labels": labels[N_LOG:], "pscores": pscores[N_LOG:]}
        return tr, va

    for layout in rc.LAYOUTS:
        XU, XI = rc.side_matrices(layout, user, item, ctx)
        train, val = split(rc.pair_rows(XU, XI, log_users, log_items))
        X_all = rc.pair_rows(XU, XI, uu, ii)
        out = {}
        for k, alpha in rc.FM_CASES:
            lr = 1e-4
            while True:
                m = FM(estimator="IPS", n_epochs=FM_ITERS, n_factors=k, n_features=XU.shape[1], lr=lr,
                       batch_size=BATCH, seed=SEED, alpha=alpha)
                m.fit(train, val)
                if np.isfinite(m.V()).all() and np.isfinite(m.w()).all() and np.isfinite(m.w0()).all():
                    break
                lr /= 10.0
            name = rc.case_name(k, alpha)
            R = np.asarray(m.predict(X_all)).reshape(nu, ni)
            out[f"{name}_lr"] = np.float64(lr)
            out[f"{name}_w0"] = m.w0().copy()
            out[f"{name}_w"] = m.w().copy()
            if k <= 33:
                out[f"{name}_V"] = m.V().copy()
            out[f"{name}_R"] = R
            # what the tests rely on: the identity holds, and how tied / saturated the case is
            logit = rc.fm_logits(XU, XI, m.w0(), m.w(), m.V())
            err = np.max(np.abs(rc.sigmoid(logit) - R)) / np.max(np.abs(R))
            top = np.sort(R, axis=1)[:, ::-1][:, :11]
            print(f"{layout} {name}: lr={lr:g} identity rel_err={err:.2e} saturated={np.mean((R == 0) | (R == 1)):.3f} "
                  f"min gap in top 10={np.min(top[:, :-1] - top[:, 1:]):.2e} max|logit|={np.max(np.abs(logit)):.1f}")
        save(f"recommend_fm_{layout}", out)

    pairs = np.stack([log_users, log_items], axis=1)
    train, val = split(pairs)
    all_pairs = np.stack([uu, ii], axis=1)
    for k in rc.MF_FACTORS:
        m = MF(estimator="IPS", n_epochs=MF_ITERS, n_factors=k, n_users=nu, n_items=ni, lr=0.02, reg=0.5,
               batch_size=BATCH, seed=SEED)
        m.fit(train, val)
        common.update({f"mf_k{k}_P": m.P().copy(), f"mf_k{k}_Q": m.Q().copy(), f"mf_k{k}_bu": m.b_u().copy(),
                       f"mf_k{k}_bi": m.b_i().copy(), f"mf_k{k}_b": np.float64(m.b),
                       f"mf_k{k}_R": np.asarray(m.predict(all_pairs)).reshape(nu, ni)})
    save("recommend", common)


if __name__ == "__main__":
    main()
