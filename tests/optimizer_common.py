"""Shared by the tests of the optimiser seam of both models (adagrad_common.py for the FM fit,
mf_adagrad_common.py for the exact MF batch step): the kinds of the C ABI, the AdaGrad rule of one
array in NumPy float64 and in long double, and the input digest the golden files carry.  Importing
this module touches neither the GPU nor the package under test.

The rule, per element with accumulator G and gradient g (include/rfm_hip.h, "the optimiser seam"):
    G_new = G + g * g,    theta_new = theta - lr * g / (sqrt(G_new) + eps)."""
import hashlib

import numpy as np

LD = np.longdouble
SGD, ADAGRAD = 0, 1   # the kinds of both optimiser seams of include/rfm_hip.h


def _rule(theta, G, g, lr, eps):
    Gn = G + g * g
    return theta - (lr * g) / (np.sqrt(Gn) + eps), Gn


def rule_f64(theta, G, g, lr, eps):
    """(theta_new, G_new) in NumPy float64: the operations the kernels run, one rounding each."""
    return _rule(*(np.asarray(a, dtype=np.float64) for a in (theta, G, g)), lr, eps)


def rule_ld(theta, G, g, lr, eps):
    """(theta_new, G_new) in long double."""
    return _rule(*(np.asarray(a).astype(LD) for a in (theta, G, g)), LD(lr), LD(eps))


def log_digest(train, val):
    """The input digest the golden generators store (tests/golden/make_golden.py log_digest), of a
    log whose ``features`` are a CSR matrix (FM) or a dense array of pairs (MF)."""
    def digest(*arrays):
        h = hashlib.sha256()
        for a in arrays:
            h.update(np.ascontiguousarray(a).tobytes())
        return h.hexdigest()

    parts = []
    for d in (train, val):
        f = d["features"]
        parts.append(digest(f.indptr.astype(np.int64), f.indices.astype(np.int64), f.data) if hasattr(f, "indptr")
                     else digest(f))
        parts.append(digest(d["labels"], d["pscores"]))
    return "|".join(parts)
