"""Build container: register figures and a digest of the gfx950 disassembly of every kernel of two builds of
rfm_pairs.o -- the pair tile in each mode and form, the merge, the ranking kernel and the rest (the per-kernel view is
profiles/kernel_isa.sh).  The parent's pair_tile_kernel<MODE> is compared with this tree's pair_tile_kernel<MODE, 0>;
the by-item form <MODE, 1> has no parent and is listed beside its forward twin.
usage: register_counts.py PARENT.o THIS.o"""
import difflib, hashlib, re, subprocess, sys, tempfile
B = "/opt/rocm/lib/llvm/bin"
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
          "group_segment_fixed_size")


def kernels(obj):
    t = tempfile.mkdtemp()
    subprocess.check_call(["cp", obj, t + "/in.o"])
    subprocess.check_call([B + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + t + "/fat.bin", t + "/in.o", t + "/out.o"])
    subprocess.check_call([B + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + t + "/fat.bin",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + t + "/dev.co"])
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
            ins = re.sub(r"//.*", "", line).strip()  # drop addresses / branch-target comments
            body[name].append(re.sub(r"^[0-9a-f]+:\s*", "", ins))
    out = {}
    for n, m in meta.items():
        dem = subprocess.check_output(["c++filt", n], text=True).strip()
        dem = re.sub(r"^void ", "", dem).replace("rfm::(anonymous namespace)::", "")
        dem = re.sub(r"\(.*\)$", "", dem)
        text = "\n".join(body.get(n, []))
        out[dem] = (m, hashlib.sha1(text.encode()).hexdigest()[:12], len(body.get(n, [])), text)
    return out


def row(tag, name, entry):
    m, h, n, _ = entry
    return f"{tag:6} {name} | " + " ".join(m.get(f, "-") for f in FIELDS) + f" | {n} | {h}"


if __name__ == "__main__":
    parent, this = kernels(sys.argv[1]), kernels(sys.argv[2])
    twin = lambda k: re.sub(r"pair_tile_kernel<(\d+), 0>", r"pair_tile_kernel<\1>", k)  # noqa: E731
    print("kernel | " + " ".join(FIELDS) + " | instructions | ISA digest")
    for k in sorted(this):
        print(row("this", k, this[k]))
        if twin(k) in parent:
            p = parent[twin(k)]
            same = p[1] == this[k][1]
            changed = sum(1 for l in difflib.unified_diff(p[3].splitlines(), this[k][3].splitlines(), n=0, lineterm="")
                          if l[:1] in "+-" and l[:3] not in ("+++", "---"))
            print(row("parent", twin(k), p) + ("  SAME ISA" if same else f"  ISA DIFFERS in {changed} lines"))
            assert all(p[0].get(f) == this[k][0].get(f) for f in FIELDS), f"{k}: a register or segment figure moved"
        else:
            print(f"       (no parent: {k})")
    missing = sorted(set(parent) - {twin(k) for k in this})
    assert not missing, missing
