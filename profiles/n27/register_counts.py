"""Build container: register figures and a digest of the gfx950 disassembly of the normalisation kernel and of both
top-K merge instantiations (rows_normalise_kernel, topk_merge_kernel<false / true>) of two builds of rfm_pairs.o (the per-kernel view is
profiles/kernel_isa.sh).  usage: register_counts.py PARENT.o THIS.o [DIR for a.s / b.s]"""
import hashlib, os, re, subprocess, sys, tempfile
B = "/opt/rocm/lib/llvm/bin"

def kernels(obj):
    t = tempfile.mkdtemp()
    subprocess.check_call(["cp", obj, t + "/in.o"])
    subprocess.check_call([B + "/llvm-objcopy", "--dump-section", ".hip_fatbin=" + t + "/fat.bin", t + "/in.o", t + "/out.o"])
    subprocess.check_call([B + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + t + "/fat.bin",
                           "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + t + "/dev.co"])
    notes = subprocess.check_output([B + "/llvm-readelf", "--notes", t + "/dev.co"], text=True)
    meta = {}
    cur = {}
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)", line)
        if not m:
            continue
        if re.match(r"\s*- \.agpr_count", line) or re.match(r"\s*- \.args", line):
            if "name" in cur:
                meta[cur["name"]] = cur
            cur = {}
        key, val = m.group(1), m.group(2).strip()
        if key in ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
                   "group_segment_fixed_size", "agpr_count"):
            cur[key] = val
        if key == "name" and val.startswith("_Z"):
            cur["name"] = val
    if "name" in cur:
        meta[cur["name"]] = cur
    dis = subprocess.check_output([B + "/llvm-objdump", "-d", "--no-show-raw-insn", t + "/dev.co"], text=True)
    body = {}
    name = None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.*)>:", line)
        if m:
            name = m.group(1)
            body[name] = []
            continue
        if name and line.strip():
            # drop addresses / branch-target comments
            ins = re.sub(r"//.*", "", line).strip()
            ins = re.sub(r"^[0-9a-f]+:\s*", "", ins)
            body[name].append(ins)
    out = {}
    for n, m in meta.items():
        if not any(w in n for w in ("rows_normalise_kernel", "topk_merge_kernel")):
            continue
        dem = subprocess.check_output(["c++filt", n], text=True).strip()
        text = "\n".join(body.get(n, []))
        out[dem] = (m, hashlib.sha1(text.encode()).hexdigest()[:12], len(body.get(n, [])), text)
    return out

if __name__ == "__main__":
    parent, this = kernels(sys.argv[1]), kernels(sys.argv[2])
    def norm(d):
        d = d.replace("topk_merge_kernel<false>", "topk_merge_kernel")  # (the parent's is no template)
        d = re.sub(r"^void ", "", d).replace("rfm::(anonymous namespace)::", "")
        return re.sub(r"\(.*\)$", "", d)
    pn = {norm(k): v for k, v in parent.items()}
    fields = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
              "group_segment_fixed_size")
    print("kernel | " + " ".join(fields) + " | instructions | ISA digest")
    for k in sorted(this):
        m, h, n, text = this[k]
        line = f"this   {norm(k)} | " + " ".join(m.get(f, "-") for f in fields) + f" | {n} | {h}"
        print(line)
        if norm(k) in pn:
            m2, h2, n2, text2 = pn[norm(k)]
            print(f"parent {norm(k)} | " + " ".join(m2.get(f, "-") for f in fields) + f" | {n2} | {h2}"
                  + ("  SAME ISA" if h == h2 else "  ISA DIFFERS in %d lines" % sum(1 for l in __import__("difflib").unified_diff(text2.splitlines(), text.splitlines(), n=0, lineterm="") if l[:1] in "+-" and l[:3] not in ("+++", "---"))))
            if h != h2 and len(sys.argv) > 3:
                open(sys.argv[3] + "/a.s", "w").write(text2); open(sys.argv[3] + "/b.s", "w").write(text)
