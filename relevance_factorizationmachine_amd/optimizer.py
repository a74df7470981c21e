"""Parameter handles with the call surface of the reference's ``SGD``
(``utils/optimizer.py:36-64``): ``h()`` returns the parameters, ``h(index)`` one
entry, ``h.update(grad, index)`` applies ``params[index] -= lr * grad``.

The parameters live in HBM and are updated by the HIP kernels; a handle only
moves them to the host when a caller asks.  ``update`` is kept for API
compatibility (the training path never calls it).

``DeviceAdaGrad`` is the same handle with a second update rule: the subclass of the reference's
``BaseOptimizer`` that keeps an accumulator per element.  The FM fit runs it
inside the gradient launch (``FactorizationMachines.optimizer = "adagrad"``), the exact MF fit inside
the level kernels (``LogisticMatrixFactorization.optimizer = "adagrad"``)."""
from __future__ import annotations

import numpy as np


class DeviceSGD:
    def __init__(self, rt, params: np.ndarray, lr: float):
        self._rt = rt
        self.lr = lr
        self._shape = params.shape
        self.dev = rt.upload(np.ascontiguousarray(params, dtype=np.float64))

    @property
    def params(self) -> np.ndarray:
        self._rt.sync()
        return self.dev.cpu().numpy()

    def __call__(self, index=None):
        p = self.params
        return p if index is None else p[index]

    def update(self, grad, index=None) -> None:
        p = self.params
        if index is None:
            p -= self.lr * grad
        else:
            p[index] -= self.lr * grad
        self.set(p)

    def append(self, dev_rows) -> None:
        """Grows the parameters by the device tensor ``dev_rows`` along the first axis (fold-in)."""
        import torch

        self.dev = torch.cat([self.dev, dev_rows.to(self.dev.dtype)], dim=0).contiguous()
        self._shape = tuple(self.dev.shape)

    def set(self, params: np.ndarray) -> None:
        host = np.ascontiguousarray(params, dtype=np.float64).reshape(self._shape)
        self.dev.copy_(self._rt.upload(host))


def adagrad_update(params: np.ndarray, acc: np.ndarray, grad, lr: float, eps: float, index=None) -> None:
    """The AdaGrad rule on host arrays, in place: ``G += g * g`` (the product rounded, then the sum),
    ``theta -= (lr * g) / (sqrt(G) + eps)`` -- NumPy float64 states the operations the kernels run
    (``include/rfm_hip.h``, "the optimiser seam")."""
    g = np.asarray(grad, dtype=np.float64)
    if index is None:
        acc += g * g
        params -= (lr * g) / (np.sqrt(acc) + eps)
    else:
        acc[index] = acc[index] + g * g
        params[index] = params[index] - (lr * g) / (np.sqrt(acc[index]) + eps)


class DeviceAdaGrad(DeviceSGD):
    """``DeviceSGD`` plus the accumulators of AdaGrad: ``acc`` (device tensor of the parameters'
    shape, float64, ``init`` everywhere at first) and ``eps``.  ``dev``: take this device tensor as
    the parameters instead of uploading ``params`` (a handle that changes its rule keeps its
    parameters where they are)."""

    def __init__(self, rt, params, lr: float, eps: float = 1e-10, init: float = 0.0, dev=None):
        import torch

        if dev is None:
            super().__init__(rt, params, lr)
        else:
            self._rt, self.lr, self._shape, self.dev = rt, lr, tuple(dev.shape), dev
        self.eps = float(eps)
        self.init = float(init)
        self.acc = torch.full(tuple(self.dev.shape), self.init, dtype=torch.float64, device=self.dev.device)

    def update(self, grad, index=None) -> None:
        p = self.params
        acc = self.acc.cpu().numpy()
        adagrad_update(p, acc, grad, self.lr, self.eps, index)
        self.set(p)
        self.acc.copy_(self._rt.upload(np.ascontiguousarray(acc)))

    def append(self, dev_rows) -> None:
        """Grows the parameters as ``DeviceSGD.append`` does, and ``acc`` by rows of ``init``."""
        import torch

        super().append(dev_rows)
        grown = torch.full((int(dev_rows.shape[0]),) + tuple(self.acc.shape[1:]), self.init, dtype=torch.float64,
                           device=self.acc.device)
        self.acc = torch.cat([self.acc, grown], dim=0).contiguous()


def take_optimizer(model, names, inexact: bool = False) -> bool:
    """Checks ``model.optimizer``; with "adagrad" the handles ``names`` of the model become
    ``DeviceAdaGrad`` on the same device tensors (once: the accumulators persist).  ``inexact``: the
    model is in a mode without a batch order (MF's ``hogwild``), which only the SGD rule runs in.
    True for AdaGrad."""
    if model.optimizer not in ("sgd", "adagrad"):
        raise ValueError(f"optimizer must be 'sgd' or 'adagrad', got {model.optimizer!r}")
    if model.optimizer == "sgd":
        return False
    if not float(model.adagrad_eps) > 0.0:
        raise ValueError(f"adagrad_eps={model.adagrad_eps!r} must be > 0")
    if inexact:
        raise ValueError("optimizer = 'adagrad' runs in exact mode only (hogwild = True has no order)")
    for name in names:
        h = getattr(model, name)
        if not isinstance(h, DeviceAdaGrad):
            setattr(model, name, DeviceAdaGrad(model._rt, None, h.lr, model.adagrad_eps, model.adagrad_init, dev=h.dev))
    return True
