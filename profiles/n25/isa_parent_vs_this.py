"""Build container: every gfx950 kernel of every object of two builds of the library, parent against this tree -- register
figures, spills, scratch, static LDS, instruction count and a digest of the disassembly (profiles/n23/register_counts.py
for all kernels of all objects).  Kernels are matched by demangled template name and template arguments, the parameter
list dropped and the parent's MfSgdRule read as SgdRule.  Exit status 1 unless every kernel of the parent has exactly one
partner with the same figures and digest and this tree has no kernel besides.  The comparison is always per kernel.  The
table prints a row per kernel for the kernels that take an update rule (the ones whose parameter type this change renames)
and for any kernel that differs; the other kernels, where both builds agree, are one row per template (the name before
`<`) with the number of kernels, the sum of their instructions and a digest over their rows; `--all` prints every row.
usage: isa_parent_vs_this.py PARENT_BUILD_DIR THIS_BUILD_DIR [--all]   (the directories of the objects, csrc/build)"""
import hashlib, os, re, subprocess, sys, tempfile
B = "/opt/rocm/lib/llvm/bin"
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size")


def strip_params(dem):
    """`void f<A, B>(X, Y)` -> `f<A, B>`: the last balanced (...) group goes."""
    dem = re.sub(r"^void ", "", dem)
    if dem.endswith(" [clone .kd]"):
        dem = dem[:-len(" [clone .kd]")]
    assert dem.endswith(")"), dem
    depth = 0
    for i in range(len(dem) - 1, -1, -1):
        depth += dem[i] == ")"
        depth -= dem[i] == "("
        if depth == 0:
            return dem[:i]
    raise ValueError(dem)


def short(name):
    name = name.replace("rfm::", "")
    return name if len(name) <= 56 else name[:56] + "#" + hashlib.sha1(name.encode()).hexdigest()[:8]


def row(d, k):
    figs, h, n = d[k]
    return f"{short(k)} | " + " ".join(figs) + f" | {n} | {h}"


def kernels(obj):
    """name without parameters -> (figures, digest, instructions) of one object; {} for an object without device code."""
    t = tempfile.mkdtemp()
    sections = subprocess.check_output([B + "/llvm-readelf", "-S", obj], text=True)
    if ".hip_fatbin" not in sections:
        return {}
    subprocess.check_call([B + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + t + "/fat.bin", obj, t + "/out.o"])
    subprocess.check_call([B + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + t + "/fat.bin",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + t + "/dev.co"])
    if os.path.getsize(t + "/dev.co") == 0:
        return {}
    notes = subprocess.check_output([B + "/llvm-readelf", "--notes", t + "/dev.co"], text=True)
    meta, cur = {}, {}
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)", line)
        if not m:
            continue
        if re.match(r"\s*- \.agpr_count", line) or re.match(r"\s*- \.args", line):
            if "name" in cur:
                meta[cur["name"]] = cur
            cur = {}
        key, val = m.group(1), m.group(2).strip()
        if key in FIELDS:
            cur[key] = val
        if key == "name" and val.startswith("_Z"):
            cur["name"] = val
    if "name" in cur:
        meta[cur["name"]] = cur
    dis = subprocess.check_output([B + "/llvm-objdump", "-d", "--no-show-raw-insn", t + "/dev.co"], text=True)
    body, name = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
        if m:
            name = m.group(1)
            body[name] = []
            continue
        if name and line.strip():
            ins = re.sub(r"//.*", "", line).strip()      # addresses and branch-target comments go
            body[name].append(re.sub(r"^[0-9a-f]+:\s*", "", ins))
    names = sorted(meta)
    dems = subprocess.check_output(["c++filt"] + names, text=True).splitlines() if names else []
    out = {}
    for n, dem in zip(names, dems):
        key = strip_params(dem.strip()).replace("MfSgdRule", "SgdRule")
        assert key not in out, key
        text = "\n".join(body[n])
        out[key] = (tuple(meta[n].get(f, "-") for f in FIELDS), hashlib.sha1(text.encode()).hexdigest()[:12], len(body[n]))
    return out


if __name__ == "__main__":
    parent_dir, this_dir, every = sys.argv[1], sys.argv[2], "--all" in sys.argv[3:]
    objects = sorted(f for f in os.listdir(parent_dir) if f.endswith(".o"))
    assert objects == sorted(f for f in os.listdir(this_dir) if f.endswith(".o")), "the builds have different objects"
    print("kernel | vgpr agpr sgpr vgpr_spill sgpr_spill scratch_bytes static_lds_bytes | instructions | ISA digest"
          "   (a row without a verdict: parent and this tree agree in all of it)")
    print("template<*> | kernels | instructions, summed | digest over the kernels' rows   (all of them agree)")
    bad = total = 0
    for obj in objects:
        parent, this = kernels(os.path.join(parent_dir, obj)), kernels(os.path.join(this_dir, obj))
        same, families = 0, {}
        print(f"## {obj}")
        for k in sorted(set(parent) | set(this)):
            total += 1
            if k in parent and k in this and parent[k] == this[k]:
                verdict = "SAME"
                same += 1
            else:
                verdict = "DIFFERS" if k in parent and k in this else ("ONLY IN PARENT" if k in parent else "ONLY IN THIS TREE")
                bad += 1
            if verdict == "SAME" and not every and "Rule" not in k:
                families.setdefault(k.split("<")[0], []).append(k)
                continue
            for side, d in (("parent", parent), ("this", this)):
                if k in d and (verdict != "SAME" or side == "this"):
                    print(row(d, k) + (f" | {verdict} ({side})" if verdict != "SAME" else ""))
        for fam, ks in sorted(families.items()):
            digest = hashlib.sha1("\n".join(row(this, k) for k in ks).encode()).hexdigest()[:12]
            print(f"{short(fam)}<*> | {len(ks)} | {sum(this[k][2] for k in ks)} | {digest}")
        print(f"# {obj}: {len(parent)} kernels in the parent, {len(this)} in this tree, {same} with the same figures and digest")
    print(f"# all objects: {total} kernels, {bad} without an identical partner")
    sys.exit(1 if bad else 0)
