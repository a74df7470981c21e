"""Generate tests/golden/fm_adagrad_coat_k8.npz by RUNNING THE REFERENCE with another optimiser.

Run in the build container only (``/root/reference`` does not exist on the GPU box)::

    python tests/golden/make_golden_adagrad.py

The reference writes its models against ``utils.optimizer.BaseOptimizer`` (``update(grad, index)``)
and ``src/fm.py`` builds ``w0``, ``w`` and ``V`` as ``SGD(params=..., lr=...)``.  This script defines
an AdaGrad subclass of the reference's ``BaseOptimizer`` (below: this project's text), assigns it
to ``src.fm.SGD`` and runs the reference's ``FactorizationMachines`` unchanged on the seeded
coat-shaped log of ``relevance_factorizationmachine_amd.synth``.  Nothing of the reference is
copied: the fixture holds the inputs' digests and the reference's numeric OUTPUTS -- final
parameters, the three accumulators, both loss lists -- for the IPS and Naive estimators.
"""
from __future__ import annotations

import os
import sys
from dataclasses import dataclass

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden as mg  # noqa: E402  (digests, save, the import of the reference)

LR, EPS, INIT, N_EPOCHS, SEED = 0.05, 1e-10, 0.0, 30, 12345


def adagrad_class(BaseOptimizer):
    """G += g * g; theta -= (lr * g) / (sqrt(G) + eps), as a subclass of the reference's seam."""

    @dataclass
    class AdaGrad(BaseOptimizer):
        def __post_init__(self):
            self.acc = np.full(np.shape(self.params), INIT, dtype=np.float64)

        def update(self, grad, index) -> None:
            grad = np.asarray(grad, dtype=np.float64)
            if index is None:
                self.acc += grad * grad
                self.params -= (self.lr * grad) / (np.sqrt(self.acc) + EPS)
            else:
                self.acc[index] = self.acc[index] + grad * grad
                self.params[index] = self.params[index] - (self.lr * grad) / (np.sqrt(self.acc[index]) + EPS)

    return AdaGrad


def main():
    FM = mg._import_reference()[0]
    import src.fm as ref_fm  # (the reference's: _import_reference left it in sys.modules)
    from utils.optimizer import BaseOptimizer

    assert ref_fm.__file__.startswith(mg.REF) and BaseOptimizer.__module__ == "utils.optimizer"
    ref_fm.SGD = adagrad_class(BaseOptimizer)
    shape = mg.synth.SHAPES["coat"]
    assert shape.n_factors == 8 and shape.batch_size == 500
    out = {}
    for est in ("IPS", "Naive"):
        train, val = mg.synth.make_log(shape, "FM", est, seed=0)
        model = FM(estimator=est, n_epochs=N_EPOCHS, n_factors=shape.n_factors,
                   n_features=train["features"].shape[1], lr=LR, batch_size=shape.batch_size, seed=SEED)
        tr, va = model.fit(train, val)
        print(f"{est}: train loss {tr[0]:.4f} -> {tr[-1]:.4f}, val loss {va[0]:.4f} -> {va[-1]:.4f}")
        out[f"{est}_train_loss"] = np.asarray(tr)
        out[f"{est}_val_loss"] = np.asarray(va)
        for name in ("w0", "w", "V"):
            out[f"{est}_{name}"] = getattr(model, name)().copy()
            out[f"{est}_acc_{name}"] = getattr(model, name).acc.copy()
        out[f"{est}_input_digest"] = np.array(mg.log_digest(train, val))
    out.update(n_epochs=np.int64(N_EPOCHS), seed=np.int64(SEED), lr=np.float64(LR), eps=np.float64(EPS),
               init=np.float64(INIT))
    mg.save("fm_adagrad_coat_k8", **out)


if __name__ == "__main__":
    main()
