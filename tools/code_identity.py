#!/usr/bin/env python3
"""Per-symbol identity of the device code two builds compiled from render.hip -- the check a refactor that must not change code is held to.
usage: python tools/code_identity.py <parent_build_dir> <branch_build_dir>      (two B= directories of pearray_amd/csrc/Makefile; no GPU)

For every render_*.o of either directory: unbundle the gfx950 code object (llvm-objdump --offloading, as tools/kernel_resources.py does),
disassemble it and hash every symbol: sha256[:16] over its instruction text (addresses, encodings and branch-target annotations stripped)
followed, for a kernel, by its descriptor's values from the code object's metadata.  One line per symbol:
    SAME|DIFF <unit> <K|f> <symbol> <parent hash> <branch hash>
(K = kernel, f = other device function; rocprim / hipcub kernels are named rocprim~<sha256[:16] of the mangled name>), a DIFF line of a kernel
is followed by both sides' descriptor values, and the last line counts: N kernels, M device functions, D differ.
Exit status: 1 when a unit or a symbol exists on one side only, else 0 (a differing symbol is reported, not judged)."""
import glob, hashlib, os, re, subprocess, sys, tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
# the kernel descriptor's values that enter a kernel's hash (metadata keys of the code object's notes)
DESC = ["vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size", "vgpr_spill_count", "sgpr_spill_count",
        "kernarg_segment_size", "max_flat_workgroup_size", "uses_dynamic_stack"]


def unit_symbols(obj):
    """{symbol: (is_kernel, hash, descriptor text)} of one host object's gfx950 code object"""
    with tempfile.TemporaryDirectory() as d:
        tmp = os.path.join(d, os.path.basename(obj))
        os.symlink(os.path.abspath(obj), tmp)
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", tmp], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=d)
        co = [f for f in glob.glob(tmp + ".*") if "gfx950" in f]
        if not co:
            sys.exit("no gfx950 code object in " + obj)
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co[0]], capture_output=True, text=True, check=True).stdout
        asm = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", co[0]], capture_output=True, text=True, check=True).stdout
    desc = {}
    for block in notes.split("- .agpr_count:")[1:]:
        block = ".agpr_count: " + block
        get = lambda key: (re.search(r"\." + key + r":\s+(\S+)", block) or [None, "-"])[1]  # noqa: E731
        desc[get("name")] = " ".join("%s=%s" % (k, get(k)) for k in DESC)
    text, name = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            text[name] = []
        elif name is not None and line.strip():
            text[name].append(re.sub(r"\s*//.*$", "", line).strip())  # drops "// address: encoding <target annotation>"
    out = {}
    for name, lines in text.items():
        kernel = name in desc
        body = "\n".join(lines) + ("\n" + desc[name] if kernel else "")
        out[name] = (kernel, hashlib.sha256(body.encode()).hexdigest()[:16], desc.get(name, ""))
    return out


def shown(sym):
    return "rocprim~" + hashlib.sha256(sym.encode()).hexdigest()[:16] if "rocprim" in sym or "hipcub" in sym else sym


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    units = [sorted(os.path.basename(p) for p in glob.glob(os.path.join(d, "render_*.o"))) for d in sys.argv[1:3]]
    one_sided = sorted(set(units[0]) ^ set(units[1]))
    for u in one_sided:
        print("ONLY-%s %s" % ("PARENT" if u in units[0] else "BRANCH", u))
    n_k = n_f = n_diff = 0
    for u in sorted(set(units[0]) & set(units[1])):
        a, b = (unit_symbols(os.path.join(d, u)) for d in sys.argv[1:3])
        unit = u[len("render_"):-len(".o")]
        for sym in sorted(set(a) | set(b), key=lambda s: (not (a.get(s) or b.get(s))[0], s)):
            if sym not in a or sym not in b:
                print("ONLY-%s %s %s %s" % ("PARENT" if sym in a else "BRANCH", unit, "K" if (a.get(sym) or b.get(sym))[0] else "f", shown(sym)))
                one_sided.append(sym)
                continue
            kernel, same = a[sym][0], a[sym][1] == b[sym][1]
            n_k += kernel
            n_f += not kernel
            n_diff += not same
            print("%s %s %s %s %s %s" % ("SAME" if same else "DIFF", unit, "K" if kernel else "f", shown(sym), a[sym][1], b[sym][1]))
            if not same and kernel:
                print("#   parent: " + a[sym][2])
                print("#   branch: " + b[sym][2])
    print("%d kernels, %d device functions, %d differ" % (n_k, n_f, n_diff))
    return 1 if one_sided else 0


if __name__ == "__main__":
    sys.exit(main())
