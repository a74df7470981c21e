"""Build container: register figures and a digest of the gfx950 disassembly of every kernel of every object of two
builds (csrc/build/*.o), read as profiles/n29/register_counts.py reads one object.  Every kernel of the parent must
be in this tree with the same figures and the same ISA digest; the kernels of rfm_diverse.o have no parent.
usage: register_counts.py PARENT/csrc/build THIS/csrc/build"""
import glob
import importlib.util
import os
import sys

spec = importlib.util.spec_from_file_location("n29", os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "n29",
                                                                  "register_counts.py"))
n29 = importlib.util.module_from_spec(spec)
spec.loader.exec_module(n29)


def build(folder):
    out = {}
    for obj in sorted(glob.glob(os.path.join(folder, "*.o"))):
        try:
            found = n29.kernels(obj)
        except Exception:  # (a host-only object has no device code)
            continue
        for name, entry in found.items():
            out[(os.path.basename(obj), name)] = entry
    return out


if __name__ == "__main__":
    parent, this = build(sys.argv[1]), build(sys.argv[2])
    print("object kernel | " + " ".join(n29.FIELDS) + " | instructions | ISA digest")
    moved = []
    for key in sorted(this):
        if key in parent:
            same = parent[key][1] == this[key][1] and all(parent[key][0].get(f) == this[key][0].get(f) for f in n29.FIELDS)
            print(n29.row("this", " ".join(key), this[key]) + ("  = parent" if same else ""))
            if not same:
                print(n29.row("parent", " ".join(key), parent[key]) + "  DIFFERS")
                moved.append(key)
        else:
            print(n29.row("this", " ".join(key), this[key]) + "  (no parent)")
    missing = sorted(set(parent) - set(this))
    print(f"{len(this)} kernels in this tree, {len(parent)} in the parent; moved: {moved or 'none'}; missing: {missing or 'none'}")
    assert not moved and not missing
