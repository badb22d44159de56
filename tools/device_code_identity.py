"""python tools/device_code_identity.py OLD_DIR NEW_DIR: is the gfx950 code of every rs_*.o the same in two builds?

Takes the gfx950 code object out of each object file's .hip_fatbin section (llvm-objcopy, clang-offload-bundler) and compares, per unit: the raw code objects, the
disassembly of every kernel (llvm-objdump -d), and the kernels' metadata notes (VGPRs, AGPRs, SGPRs, scratch, LDS, as
tools/kernel_meta.py reports them).  For refactors of host code: the argument that kernel speed cannot have moved."""
import hashlib, os, re, subprocess, sys, tempfile
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def code_object(obj, tmp):
    out = os.path.join(tmp, os.path.basename(obj) + "." + hashlib.md5(obj.encode()).hexdigest()[:6] + ".co")
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + out + ".fatbin", obj], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--input=" + out + ".fatbin", "--output=" + out], check=True)
    return out


def describe(co):
    raw = hashlib.sha256(open(co, "rb").read()).hexdigest()[:12]
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co], capture_output=True, text=True, check=True).stdout
    dis = "\n".join(dis.splitlines()[2:])                                  # (the first lines name the file)
    notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True, check=True).stdout
    meta = {}
    for blk in notes.split("  - .agpr_count:")[1:]:
        blk = ".agpr_count:" + blk
        g = lambda k: (re.search(r"\.%s:\s+(\S+)" % k, blk) or [None, "?"])[1]      # noqa: E731
        meta[g("name")] = tuple(g(k) for k in KEYS)
    return raw, dis, meta


old, new = sys.argv[1], sys.argv[2]
bad = 0
with tempfile.TemporaryDirectory() as tmp:
    for f in sorted(x for x in os.listdir(new) if x.startswith("rs_") and x.endswith(".o")):
        a, b = describe(code_object(os.path.join(old, f), tmp)), describe(code_object(os.path.join(new, f), tmp))
        same_dis, same_meta = a[1] == b[1], a[2] == b[2]
        bad += not (same_dis and same_meta)
        print(f"{f:22s} kernels {len(b[2]):4d}  code object {a[0]} | {b[0]} {'same' if a[0] == b[0] else 'DIFFERS'}  "
              f"disassembly {hashlib.sha256(b[1].encode()).hexdigest()[:12]} {'same' if same_dis else 'DIFFERS'}  "
              f"vgpr/agpr/sgpr/scratch/lds {'same' if same_meta else 'DIFFERS'}")
        for k in sorted(set(a[2]) | set(b[2])):
            if a[2].get(k) != b[2].get(k):
                print("    ", k, a[2].get(k), "->", b[2].get(k))
print("identical device code" if not bad else f"{bad} unit(s) differ")
sys.exit(1 if bad else 0)
