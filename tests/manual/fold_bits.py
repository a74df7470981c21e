#!/usr/bin/env python3
"""What fold-in leaves behind, in one .npz, to compare two trees (kernels, entries and test helpers)
bit for bit: every listed case of fold_in_common.py and of fm_fold_common.py, and MF's ``grid_case``
of the device, through the raw ABI (``run_fold``).  Kept per case: MF ``rows, bias``; FM ``w, V, A, L``.
Both kernels are free of atomics, so every array must repeat.

usage (GPU box), the other tree being e.g. a ``git worktree`` of the parent commit:
  RFM_LIB_PATH=<other tree>/relevance_factorizationmachine_amd/librfm_hip.so \\
      python tests/manual/fold_bits.py --root <other tree> --out a.npz
  python tests/manual/fold_bits.py --out b.npz
  python tests/manual/fold_bits.py --compare a.npz b.npz
``--root DIR``: the tree whose package and test helpers are imported (default: this one); the library
is that tree's own unless RFM_LIB_PATH names another (the ABI is the same).
``--compare A B`` asserts equal bits key by key."""
import argparse
import os
import sys

import numpy as np


def dump(path):
    import torch

    import fm_fold_common as fm
    import fold_in_common as mf
    import relevance_factorizationmachine_amd as pkg
    from relevance_factorizationmachine_amd import _lib, runtime

    print("package:", os.path.dirname(pkg.__file__), "library:", _lib.LIB_PATH, flush=True)
    rt = runtime.Runtime.get()
    n_cu = int(torch.cuda.get_device_properties(rt.device).multi_processor_count)
    out = {}
    for case in list(mf.fold_cases().values()) + [mf.grid_case(n_cu)]:
        out[f"mf/{case.name}/rows"], out[f"mf/{case.name}/bias"] = mf.run_fold(rt, case)
    print(f"mf: {len(mf.fold_cases()) + 1} cases", flush=True)
    for case in fm.fold_cases().values():
        for key, a in zip(("V", "w", "A", "L"), fm.run_fold(rt, case)):
            out[f"fm/{case.name}/{key}"] = a
    print(f"fm: {len(fm.fold_cases())} cases", flush=True)
    np.savez(path, **out)
    print(f"{len(out)} arrays -> {path}")


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    assert sorted(a.files) == sorted(b.files), "the two files hold different keys"
    differ = [key for key in a.files
              if a[key].shape != b[key].shape or not np.array_equal(a[key].view(np.uint64), b[key].view(np.uint64))]
    print(f"{len(a.files)} arrays, {len(a.files) - len(differ)} bit-identical in both files")
    for key in differ:
        print(f"differs: {key}")
    assert not differ, f"{len(differ)} arrays differ"


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
    args = ap.parse_args()
    if args.compare:
        compare(*args.compare)
    else:
        root = os.path.abspath(args.root)
        sys.path[:0] = [root, os.path.join(root, "tests")]
        dump(args.out)
