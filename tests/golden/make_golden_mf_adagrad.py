"""Generate tests/golden/mf_adagrad_small.npz by RUNNING THE REFERENCE with another optimiser.

Run in the build container only (``/root/reference`` does not exist on the GPU box)::

    python tests/golden/make_golden_mf_adagrad.py

The reference writes its models against ``utils.optimizer.BaseOptimizer`` (``update(grad, index)``)
and ``src/mf.py`` builds ``P``, ``Q``, ``b_u`` and ``b_i`` as ``SGD(params=..., lr=...)``.  This
script takes the AdaGrad subclass of the reference's ``BaseOptimizer`` that
``make_golden_adagrad.py`` defines (this project's text), assigns it to ``src.mf.SGD`` and runs the
reference's ``LogisticMatrixFactorization`` unchanged on the seeded kuairec_small-shaped log of
``relevance_factorizationmachine_amd.synth``: k = 16, B = 2 000, reg = 0.5, 5 iterations.  Nothing
of the reference is copied: the fixture holds the inputs' digests and the reference's numeric
OUTPUTS -- final parameters, the four accumulators, the global bias, both loss lists -- for the IPS
estimator; ``mf_adagrad_small_naive.npz`` holds the same of the Naive estimator (eight arrays of a
model of 1 411 users and 3 327 items do not compress: one file per estimator stays under 1 MiB).
"""
from __future__ import annotations

import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (digests, save, the import of the reference)
import make_golden_adagrad as mga  # noqa: E402  (the subclass, EPS, INIT)

# (lr: with G0 = 0 an element's first step is lr * sign(g); 0.05 on rows drawn in +-2.4 lets the
# train loss fall from the first iteration on -- the losses are printed)
LR, REG, N_EPOCHS, SEED, K, BATCH = 0.05, 0.5, 5, 12345, 16, 2000
NAMES = ("P", "Q", "b_u", "b_i")


def main():
    MF = mg._import_reference()[1]
    import src.mf as ref_mf  # (the reference's: _import_reference left it in sys.modules)
    from utils.optimizer import BaseOptimizer

    assert ref_mf.__file__.startswith(mg.REF) and BaseOptimizer.__module__ == "utils.optimizer"
    ref_mf.SGD = mga.adagrad_class(BaseOptimizer)
    shape = mg.synth.SHAPES["kuairec_small"]
    for est, fixture in (("IPS", "mf_adagrad_small"), ("Naive", "mf_adagrad_small_naive")):
        out = {}
        train, val = mg.synth.make_log(shape, "MF", est, seed=0)
        model = MF(estimator=est, n_epochs=N_EPOCHS, n_factors=K, n_users=shape.n_users, n_items=shape.n_items,
                   lr=LR, reg=REG, batch_size=BATCH, seed=SEED)
        tr, va = model.fit(train, val)
        print(f"{est}: train loss " + " ".join(f"{v:.4f}" for v in tr) + " | val loss " + " ".join(f"{v:.4f}" for v in va))
        out[f"{est}_train_loss"] = np.asarray(tr)
        out[f"{est}_val_loss"] = np.asarray(va)
        for name in NAMES:
            out[f"{est}_{name}"] = getattr(model, name)().copy()
            out[f"{est}_acc_{name}"] = getattr(model, name).acc.copy()
        out[f"{est}_b"] = np.float64(model.b)
        out[f"{est}_input_digest"] = np.array(mg.log_digest(train, val))
        out.update(n_epochs=np.int64(N_EPOCHS), seed=np.int64(SEED), lr=np.float64(LR), reg=np.float64(REG),
                   eps=np.float64(mga.EPS), init=np.float64(mga.INIT), n_factors=np.int64(K),
                   batch_size=np.int64(BATCH))
        mg.save(fixture, **out)


if __name__ == "__main__":
    main()
