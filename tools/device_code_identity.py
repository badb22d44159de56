"""python tools/device_code_identity.py OLD_DIR NEW_DIR: is the gfx950 code of every kernel the same in two builds?

Takes the gfx950 code object out of each rs_*.o's .hip_fatbin section (llvm-objcopy, clang-offload-bundler) and compares PER KERNEL
NAME OVER THE UNION OF ALL UNITS: the disassembly of every kernel (llvm-objdump -d, addresses and branch targets taken relative to the
kernel's first instruction and the padding behind its last one dropped, so that a kernel may change its place or its unit) and its metadata notes (VGPRs, AGPRs, SGPRs, scratch,
LDS, as tools/kernel_meta.py reports them); the two sets of kernel names must be equal, and no name may appear in two units of one
side.  A unit present on both sides also gets a line of its own (raw code object, whole disassembly, metadata).  Exit status 1 on
any difference.  For refactors of host code: the argument that kernel speed cannot have moved."""
import hashlib, os, re, subprocess, sys, tempfile
LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/llvm/bin")
KEYS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def code_object(obj, tmp):
    out = os.path.join(tmp, os.path.basename(obj) + "." + hashlib.md5(obj.encode()).hexdigest()[:6] + ".co")
    sections = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "-S", obj], capture_output=True, text=True, check=True).stdout
    if ".hip_fatbin" not in sections:
        return None                                                        # (a host-only unit)
    subprocess.run([os.path.join(LLVM, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + out + ".fatbin", obj], check=True)
    subprocess.run([os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    "--input=" + out + ".fatbin", "--output=" + out], check=True)
    return out


def per_symbol(dis):
    """{symbol: its instructions, one per line, position-independent}: `<address> <name>:` opens a symbol; an instruction line ends in
    `// <address>: <encoding>`, and a branch names its target as `<name+0xoffset>` — both are rebased on the symbol's own start."""
    out, name, base = {}, None, 0
    for line in dis.splitlines():
        m = re.match(r"^([0-9a-fA-F]+) <(.+)>:$", line)
        if m:
            base, name = int(m.group(1), 16), m.group(2)
            out[name] = []
            continue
        if name is None or not line.strip():
            continue
        m = re.match(r"^(.*?)//\s*([0-9a-fA-F]+):(.*)$", line)
        if m:
            line = "%s// +%x:%s" % (m.group(1), int(m.group(2), 16) - base, m.group(3))
        out[name].append(line)
    for v in out.values():      # what fills the gap up to the next symbol, or the end of the section, is not the kernel's
        while v and v[-1].split("//")[0].strip() in ("s_nop 0", "s_code_end", "..."):      # ("...": llvm-objdump's line for a run of zeros)
            v.pop()
    return {k: "\n".join(v) for k, v in out.items()}


def describe(co):
    if co is None:
        return "(host only)", "", {}
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


def units(d):
    return sorted(x for x in os.listdir(d) if x.startswith("rs_") and x.endswith(".o"))


def kernels_of(d, tmp, described):
    """{kernel name: (unit, disassembly, metadata)} over every unit of a build; a name defined twice is reported"""
    table, twice = {}, []
    for f in units(d):
        raw, dis, meta = described[(d, f)] = describe(code_object(os.path.join(d, f), tmp))
        code = per_symbol(dis)
        for k, m in meta.items():
            if k in table:
                twice.append((k, table[k][0], f))
            table[k] = (f, code.get(k), m)
    return table, twice


old, new = sys.argv[1], sys.argv[2]
bad = 0
with tempfile.TemporaryDirectory() as tmp:
    described = {}
    (ka, twice_a), (kb, twice_b) = kernels_of(old, tmp, described), kernels_of(new, tmp, described)
    for f in units(new):
        if (old, f) not in described:
            print(f"{f:22s} kernels {len(described[(new, f)][2]):4d}  (a unit of the new build only: its kernels are compared by name below)")
            continue
        a, b = described[(old, f)], described[(new, f)]
        same_dis, same_meta = a[1] == b[1], a[2] == b[2]
        print(f"{f:22s} kernels {len(b[2]):4d}  code object {a[0]} | {b[0]} {'same' if a[0] == b[0] else 'DIFFERS'}  "
              f"disassembly {hashlib.sha256(b[1].encode()).hexdigest()[:12]} {'same' if same_dis else 'DIFFERS'}  "
              f"vgpr/agpr/sgpr/scratch/lds {'same' if same_meta else 'DIFFERS'}")
    for f in units(old):
        if (new, f) not in described:
            print(f"{f:22s} kernels {len(described[(old, f)][2]):4d}  (a unit of the old build only)")
    for side, twice in (("old", twice_a), ("new", twice_b)):
        for k, f1, f2 in twice:
            bad += 1
            print(f"     {k}: defined in two units of the {side} build ({f1}, {f2})")
    for k in sorted(set(ka) | set(kb)):
        if k not in ka or k not in kb:
            bad += 1
            print("    ", k, "only in the", "new" if k in kb else "old", "build:", (kb.get(k) or ka.get(k))[0])
            continue
        (fa, da, ma), (fb, db, mb) = ka[k], kb[k]
        if fa != fb:
            print("    ", k, "moved:", fa, "->", fb)
        if da is None or db is None or da != db:
            bad += 1
            print("    ", k, "disassembly DIFFERS" if da is not None and db is not None else "has no code under its name")
        if ma != mb:
            bad += 1
            print("    ", k, "vgpr/agpr/sgpr/scratch/lds", ma, "->", mb)
    print(f"kernels: {len(ka)} old, {len(kb)} new, compared by name over all units")
print("identical device code" if not bad else f"{bad} difference(s)")
sys.exit(1 if bad else 0)
