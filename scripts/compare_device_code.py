"""Device code of two builds, function by function: python scripts/compare_device_code.py PARENT BRANCH
PARENT and BRANCH are two directories holding the same file names: host objects (*.o, as csrc/_obj of a checkout after make; the
gfx950 code object is taken out of each) and / or device assembly (*.s, as scripts/offline_plugin_isa.py writes with OUT_DIR).
Per file the functions are compared as text -- demangled, addresses and encodings dropped (branch operands are relative), kernel
descriptor directives and the metadata note included -- and every function that differs is listed with instructions / VGPR / AGPR /
SGPR / private segment / LDS, parent -> branch.  Exit status 1 if anything differs."""
import os, re, subprocess, sys, tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def run(*cmd):
    return subprocess.run(cmd, check=True, capture_output=True, text=True).stdout


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
    return dict(zip(names, out.stdout.split("\n")))


def from_object(path, tmp):
    """{function: [text lines]} and {kernel: {key: value}} of the gfx950 code object inside a host object"""
    fb, co = os.path.join(tmp, "fb"), os.path.join(tmp, "co")
    try:
        run(os.path.join(LLVM, "llvm-objcopy"), "--dump-section", f".hip_fatbin={fb}", path, os.path.join(tmp, "copy.o"))
    except subprocess.CalledProcessError:
        return None, None  # a host-only object
    run(os.path.join(LLVM, "clang-offload-bundler"), "--unbundle", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
        f"--input={fb}", f"--output={co}")
    funcs, cur = {}, None
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-d", "--demangle", co).split("\n"):
        m = re.match(r"^[0-9a-f]+ <(.*)>:$", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
        elif cur is not None and line.startswith("\t"):
            cur.append(re.sub(r"\s*//.*$", "", line).strip())
    # descriptors: the 64 bytes behind every <kernel>.kd symbol
    kd = {}
    for line in run(os.path.join(LLVM, "llvm-objdump"), "-D", "-j", ".rodata", "--demangle", co).split("\n"):
        m = re.match(r"^[0-9a-f]+ <(.*)\.kd>:$", line)
        if m:
            cur = kd.setdefault(m.group(1), [])
        elif re.match(r"^[0-9a-f]+ <", line):
            cur = None
        elif cur is not None and line.startswith("\t"):
            cur.append(re.sub(r"\s*//.*$", "", line).strip())
    for k, v in kd.items():
        funcs.setdefault(k, []).extend(["descriptor:"] + v)
    return funcs, metadata(run(os.path.join(LLVM, "llvm-readelf"), "--notes", co), funcs)


def metadata(text, funcs):
    """the per-kernel blocks of the amdhsa.kernels note; appended to the function's text as well"""
    meta = {}
    blocks = re.split(r"\n\s+- \.agpr_count:", text)
    for blk in blocks[1:]:
        blk = ".agpr_count:" + blk
        name = re.search(r"\.name:\s+'?([^'\n]+)'?", blk).group(1)
        meta[name] = {k: re.search(rf"\{k}:\s+(\S+)", blk).group(1) for k in KEYS}
        meta[name]["text"] = [l.strip() for l in blk.split("\n") if re.match(r"\s+\.(\w+):\s+\S", l)
                              and not re.match(r"\s+\.(name|symbol):", l)]
    dm = demangle(list(meta))
    out = {}
    for name, v in meta.items():
        d = dm[name]
        if d in funcs:
            funcs[d].extend(["metadata:"] + v.pop("text"))
        out[d] = v
    return out


def from_asm(path):
    text = open(path).read()
    funcs, meta, names = {}, {}, re.findall(r"^\s+\.amdhsa_kernel (\S+)", text, re.M)
    dm = demangle(names)
    for n in names:
        body = re.search(rf"^{re.escape(n)}:[^\n]*\n(.*?)^\s+\.end_amdhsa_kernel", text, re.S | re.M).group(1)
        lines = [re.sub(r"\s*;.*$", "", l).strip() for l in body.split("\n")]
        lines = [re.sub(r"\.LBB\d+_", ".LBB_", l) for l in lines if l and not l.startswith((".p2align", ".section", ".Lfunc_end", ".size"))]
        funcs[dm[n]] = lines
        g = lambda key: (re.search(rf"\.amdhsa_{key} (\S+)", body) or [None, "?"])[1]
        acc = g("accum_offset")
        meta[dm[n]] = {".vgpr_count": g("next_free_vgpr"), ".agpr_count": f"acc@{acc}", ".sgpr_count": g("next_free_sgpr"),
                       ".private_segment_fixed_size": g("private_segment_fixed_size"), ".group_segment_fixed_size": g("group_segment_fixed_size")}
    return funcs, meta


def ninstr(lines):
    n = 0
    for l in lines:
        if l in ("descriptor:", "metadata:") or l.startswith(".amdhsa_kernel"):
            break
        if not l.endswith(":") and not l.startswith("."):
            n += 1
    return n


def main():
    pa, br = sys.argv[1], sys.argv[2]
    total = same = 0
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for f in sorted(os.listdir(pa)):
            if not f.endswith((".o", ".s")) or not os.path.exists(os.path.join(br, f)):
                continue
            if f.endswith(".o"):
                (fa, ma), (fb, mb) = from_object(os.path.join(pa, f), tmp), from_object(os.path.join(br, f), tmp)
                if fa is None:
                    continue
            else:
                (fa, ma), (fb, mb) = from_asm(os.path.join(pa, f)), from_asm(os.path.join(br, f))
            names = sorted(set(fa) | set(fb))
            ok = [n for n in names if fa.get(n) == fb.get(n)]
            total += len(names)
            same += len(ok)
            print(f"{f:36s} {len(ok):4d} of {len(names):4d} identical")
            for n in names:
                if n in ok:
                    continue
                if n not in fa or n not in fb:
                    rows.append((f, n, "only in " + ("branch" if n in fb else "parent")))
                    continue
                a, b = ma.get(n, {}), mb.get(n, {})
                cols = [f"{ninstr(fa[n])} -> {ninstr(fb[n])}"] + [f"{a.get(k, '-')} -> {b.get(k, '-')}" for k in KEYS]
                rows.append((f, n, " | ".join(cols)))
    print(f"total: {same} of {total} identical")
    if rows:
        print("differing: file | function | instructions | VGPR | AGPR | SGPR | private segment | LDS   (parent -> branch)")
        for f, n, c in rows:
            print(f"| {f} | `{n}` | {c} |")
    return 0 if same == total else 1


if __name__ == "__main__":
    sys.exit(main())
