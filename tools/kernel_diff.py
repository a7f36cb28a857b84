"""Is the device code of a .hip file the same in two versions?  Kernel by kernel, not line by line: the order of the functions
in the assembly follows the order in which templates are instantiated, which a host-side change may move.
    python tools/kernel_diff.py OLD NEW        OLD, NEW: a .hip file (compiled device-only with the Makefile's flags, next to its
                                               own includes) or the .s of such a compile
For every function (kernels and the device functions they call) the instruction text between its label and its .Lfunc_end,
the kernel descriptor (.amdhsa_kernel block) and the amdhsa.kernels metadata entry must be equal, local label numbers
normalised.  Symbols are matched by their demangled names without "(anonymous namespace)::"; a kernel that moved into or out of
the anonymous namespace is reported, not counted as a difference.  Exit status 1 if anything differs."""
import os, re, subprocess, sys, tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-munsafe-fp-atomics",
         "-I" + os.path.join(ROOT, "include"), "-Wall", "-Wno-unused-function", "--offload-device-only", "-S"]


def assembly(path):
    if not path.endswith(".hip"):
        return open(path).read()
    with tempfile.TemporaryDirectory() as d:
        s = os.path.join(d, "a.s")
        subprocess.run(["/opt/rocm/bin/hipcc"] + FLAGS + ["-I" + os.path.dirname(os.path.abspath(path)), "-o", s, path], check=True)
        return open(s).read()


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    return dict(zip(names, out))


def normalise(text, plain):
    text = re.sub(r"\.L(func_end|func_begin|JTI|tmp)\d+(_\d+)?", lambda m: ".L" + m.group(1) + (m.group(2) or ""), text)
    text = re.sub(r"BB\d+_(\d+)", r"BB_\1", text)  # .LBB<function>_<block>, in labels and in the loop comments
    text = re.sub(r"[ \t]+;", " ;", text)  # a comment's column moves with the width of the function number in the label before it
    for sym, name in sorted(plain.items(), key=lambda kv: -len(kv[0])):  # a symbol's own spelling (namespace and all) is no difference
        text = text.replace(sym, "<" + name + ">")
    return text.strip()  # (the last metadata entry of a file ends without the blank line the others have)


def parse(txt):
    """{plain name: (demangled name, is kernel, body, descriptor, metadata)}"""
    funcs = re.findall(r"^\s*\.type\s+(\S+),@function", txt, re.M)
    kernels = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", txt, re.M))
    full = demangle(funcs)
    # without the namespace, "void " and the argument list (a symbol with C linkage has none)
    plain = {f: re.sub(r"^void |\(.*\)$", "", full[f].replace("(anonymous namespace)::", "")) for f in funcs}
    meta = {}
    for block in txt.split("  - .agpr_count:")[1:]:
        block = block.split("\namdhsa.target:")[0]
        meta[re.search(r"\.symbol:\s+(\S+)\.kd", block).group(1)] = normalise(block, plain)
    out = {}
    for f in funcs:
        # from the line after the label to the kernel descriptor's section (kernels) or the end of the function
        body = re.search(r"^" + re.escape(f) + r":[^\n]*\n(.*?)^(\s*\.section|\.Lfunc_end\d+:)", txt, re.M | re.S).group(1)
        desc = re.search(r"^\s*\.amdhsa_kernel\s+" + re.escape(f) + r"\n.*?\.end_amdhsa_kernel", txt, re.M | re.S)
        out[plain[f]] = (full[f], f in kernels, normalise(body, plain), normalise(desc.group(0), plain) if desc else "", meta.get(f, ""))
    return out


def main():
    old, new = parse(assembly(sys.argv[1])), parse(assembly(sys.argv[2]))
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(("only in NEW: " if name in new else "only in OLD: ") + name)
            bad += 1
            continue
        o, n = old[name], new[name]
        if o[0] != n[0]:
            print(f"renamed: {o[0]}  ->  {n[0]}")
        for what, a, b in (("instructions", o[2], n[2]), ("kernel descriptor", o[3], n[3]), ("metadata", o[4], n[4])):
            if a != b:
                print(f"DIFFERENT {what}: {name}")
                bad += 1
    nk = lambda d: sum(1 for v in d.values() if v[1])
    print(f"kernel_diff: {nk(old)} kernels / {len(old)} functions in OLD, {nk(new)} / {len(new)} in NEW: "
          + ("instructions, descriptors and metadata identical" if not bad else f"{bad} DIFFERENCES"))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
