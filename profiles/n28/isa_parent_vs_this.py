"""Build container: every gfx950 kernel of every object of two builds of the library, parent against this tree -- register
figures, spills, scratch, static LDS, instruction count and a digest of the disassembly (kernels() of
profiles/n25/isa_parent_vs_this.py).  The parent's forward kernels are matched through an explicit map of their names:
fm_forward_kernel<LPR, VEC, NC, BLOCK, R, REC, ELL, DET, SEG, XTRA> -> fm_forward_kernel<LPR, VEC, NC, BLOCK, (FwdKind)kind>,
R required to be what forward_rows gives, and the alias <8, 2, 2, 1024, 1, true, true, false, false, false> ->
fm_forward_lanes8_kernel<1024>; a parent's tuple that is no form of FwdKind stops the comparison.  Every other kernel is
matched by its name.  Exit status 1 unless every kernel of the parent has exactly one partner with the same figures and
digest and this tree has no kernel besides.  The table prints a row per forward kernel (the parent's name, this tree's
name, this tree's row) and per kernel that differs; the other kernels are one row per template, as in profiles/n25.
usage: isa_parent_vs_this.py PARENT_BUILD_DIR THIS_BUILD_DIR   (the directories of the objects, csrc/build)"""
import hashlib, os, re, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "n25"))
from isa_parent_vs_this import kernels, row, short  # noqa: E402

KINDS = ("kCsr", "kCsrPair", "kRecords", "kBlocks", "kRecordsFixed", "kBlocksFixed", "kRecordsRiders", "kBlocksRiders")
# (REC, ELL, DET, SEG, XTRA) -> FwdKind
KIND_OF = {(False, False, False, False, False): 0, (False, False, False, True, False): 1,
           (True, False, False, False, False): 2, (True, True, False, False, False): 3,
           (True, False, True, False, False): 4, (True, True, True, False, False): 5,
           (True, False, False, False, True): 6, (True, True, False, False, True): 7}
BIG, FWD_ROWS = 1024, 2   # kBigBlock, kFwdRows == kFwdRowsPlain


def new_name(old):
    """The parent's kernel name -> this tree's."""
    m = re.fullmatch(r"rfm::fm_forward_kernel<(\d+), (\d+), (\d+), (\d+), (\d+), (\w+), (\w+), (\w+), (\w+), (\w+)>", old)
    if not m:
        return old
    lpr, vec, nc, block, r = (int(g) for g in m.groups()[:5])
    flags = tuple(g == "true" for g in m.groups()[5:])
    if (lpr, vec, nc, block, r) == (8, 2, 2, BIG, 1) and flags == (True, True, False, False, False):
        return f"rfm::fm_forward_lanes8_kernel<{BIG}>"
    assert r == (FWD_ROWS if block == BIG and nc == 1 else 1), old
    return f"rfm::fm_forward_kernel<{lpr}, {vec}, {nc}, {block}, (rfm::FwdKind){KIND_OF[flags]}>"


if __name__ == "__main__":
    parent_dir, this_dir = sys.argv[1], sys.argv[2]
    objects = sorted(f for f in os.listdir(parent_dir) if f.endswith(".o"))
    assert objects == sorted(f for f in os.listdir(this_dir) if f.endswith(".o")), "the builds have different objects"
    print("kernel | vgpr agpr sgpr vgpr_spill sgpr_spill scratch_bytes static_lds_bytes | instructions | ISA digest"
          "   (a row without a verdict: parent and this tree agree in all of it)")
    print("parent's forward kernel -> this tree's (FwdKind: " + ", ".join(f"{i} {n}" for i, n in enumerate(KINDS)) + ")")
    print("template<*> | kernels | instructions, summed | digest over the kernels' rows   (all of them agree)")
    bad = total = 0
    for obj in objects:
        parent, this = kernels(os.path.join(parent_dir, obj)), kernels(os.path.join(this_dir, obj))
        mapped = {}
        for k in parent:
            assert new_name(k) not in mapped, k
            mapped[new_name(k)] = k
        same, families = 0, {}
        print(f"## {obj}")
        for k in sorted(set(mapped) | set(this)):
            total += 1
            old = mapped.get(k)
            if old is not None and k in this and parent[old] == this[k]:
                same += 1
                if old == k:
                    families.setdefault(k.split("<")[0], []).append(k)
                else:
                    print(f"{old.replace('rfm::', '')} -> " + row(this, k).replace("(FwdKind)", ""))
                continue
            bad += 1
            if old is not None:
                print(row(parent, old) + (" | DIFFERS (parent)" if k in this else " | ONLY IN PARENT"))
            if k in this:
                print(row(this, k) + (" | DIFFERS (this)" if old is not None else " | ONLY IN THIS TREE"))
        for fam, ks in sorted(families.items()):
            digest = hashlib.sha1("\n".join(row(this, k) for k in ks).encode()).hexdigest()[:12]
            print(f"{short(fam)}<*> | {len(ks)} | {sum(this[k][2] for k in ks)} | {digest}")
        print(f"# {obj}: {len(parent)} kernels in the parent, {len(this)} in this tree, {same} with the same figures and digest")
    print(f"# all objects: {total} kernels, {bad} without an identical partner")
    sys.exit(1 if bad else 0)
