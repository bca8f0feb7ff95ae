"""Per-kernel static comparison of two gfx950 assembly files of the same source, before / after a change that should move code only:

    hipcc <the product's flags> --cuda-device-only -S csrc/nf_gemm.hip -o before.s      (and after.s from the changed source)
    python tools/asm_compare.py [--one-workgroup-per-cu THREADS] before.s after.s [more pairs ...] > profiles/<name>.txt

Per kernel: matrix (v_mfma), LDS (ds_), barrier, global + buffer (glb), scratch (scr: spills and their reloads) and other vector-ALU
instruction counts, VGPRs, scratch bytes and occupancy from the kernel's metadata comments.  GATED (exit status 1): the two files
have the same kernel symbols; MFMA, LDS, barrier counts and occupancy are equal per kernel; global + scratch counts are equal unless
the kernel's scratch bytes moved.  VGPRs, scratch bytes and VALU counts are reported only: register allocation moves them without a
change in the work.

--one-workgroup-per-cu THREADS: the kernels are launched as at most ONE workgroup of THREADS threads per CU (the GEMM coupling
kernels: grid = min(B, CUs), 512 threads, because a workgroup takes most of a CU's LDS).  Then a SIMD never holds more than
THREADS / 64 / 4 wavefronts whatever the register count would allow, and the occupancy that is compared is
min(compiler's occupancy, THREADS / 64 / 4) — the wavefronts that are resident; the compiler's figure is still printed.

--exact before.s after.s: for a refactor that must not move a single instruction.  Kernels are matched by name; per kernel the
whole instruction text and the .amdhsa_* block (registers, scratch, LDS, next_free_*) are compared after the labels that carry the
function's ordinal in the module have been renumbered.  Prints the kernels only in `before` (instantiations the change removed),
those only in `after`, and every kernel that differs with its first differing line; exit status 1 if any kernel differs or
`after` has a kernel that `before` has not."""
import re
import subprocess
import sys


def kernels(path):
    """{symbol: {count / metadata name: int}} of every .amdhsa_kernel of an assembly file."""
    text = open(path).read()
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M)
    out = {}
    for name in names:
        start = text.index("\n%s:" % name)
        end = text.index(".end_amdhsa_kernel", start)
        info = text[end:text.index("; Occupancy:", end) + 40]
        ops = re.findall(r"^\s+([a-z][a-z0-9_]+)", text[start:text.index(".amdhsa_kernel", start)], re.M)
        row = {"mfma": 0, "lds": 0, "barrier": 0, "glb": 0, "scr": 0, "valu": 0}
        for op in ops:
            if op.startswith("v_mfma") or op.startswith("v_smfma"):
                row["mfma"] += 1
            elif op.startswith("ds_"):
                row["lds"] += 1
            elif op == "s_barrier":
                row["barrier"] += 1
            elif op.startswith(("global_", "buffer_", "flat_")):
                row["glb"] += 1
            elif op.startswith("scratch_"):
                row["scr"] += 1
            elif op.startswith("v_"):
                row["valu"] += 1
        for key, pat in (("vgpr", r"; NumVgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"), ("occ", r"; Occupancy: (\d+)")):
            row[key] = int(re.search(pat, info).group(1))
        out[name] = row
    return out


def exact_kernels(text):
    """{symbol: [lines]} of every .amdhsa_kernel of an assembly text: its instructions and labels from `symbol:` to its
    .Lfunc_end, then its .amdhsa_* block, without comments and with what depends on the function's ordinal in the module
    (.LBB<n>_, .Lfunc_begin<n>, .Lfunc_end<n>, .Ltmp<n>) renumbered: a removed instantiation elsewhere shifts those numbers."""
    out = {}
    for name in re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M):
        start = text.index("\n%s:" % name) + 1
        end = re.compile(r"^\.Lfunc_end\d+:", re.M).search(text, start).end()
        meta = text.index(".amdhsa_kernel %s\n" % name)
        body = text[start:end] + "\n" + text[meta:text.index(".end_amdhsa_kernel", meta)]
        tmp = {}
        lines = []
        for line in body.split("\n"):
            line = line.split(";")[0].strip()
            if not line or line.startswith(".ident"):
                continue
            line = re.sub(r"\.LBB\d+_", ".LBB_", line)
            line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
            line = re.sub(r"\.Ltmp\d+", lambda m: ".Ltmp%d" % tmp.setdefault(m.group(0), len(tmp)), line)
            lines.append(" ".join(line.split()))
        out[name] = lines
    return out


def exact(before, after):
    """--exact: kernel by kernel (matched by name, whatever their order), the full instruction text and the .amdhsa_* block."""
    a, b = exact_kernels(open(before).read()), exact_kernels(open(after).read())
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    common = sorted(set(a) & set(b))

    def demangle(names):
        return subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n") if names else []
    print("== exact: %s -> %s: %d / %d kernels, %d in both" % (before.split("/")[-1], after.split("/")[-1], len(a), len(b), len(common)))
    print("only in %s: %d" % (before.split("/")[-1], len(only_a)))
    for dem in demangle(only_a):
        print("    " + dem)
    print("only in %s: %d" % (after.split("/")[-1], len(only_b)))
    for dem in demangle(only_b):
        print("    " + dem)
    differ = 0
    for name, dem in zip(common, demangle(common)):
        x, y = a[name], b[name]
        if x == y:
            continue
        differ += 1
        i = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
        print("DIFFERS %s\n    line %d of %d / %d: %r -> %r" % (dem, i + 1, len(x), len(y), x[i] if i < len(x) else None, y[i] if i < len(y) else None))
    print("instruction lines compared: %d" % sum(len(a[n]) for n in common))
    print("RESULT: %d kernels in both, %d different, %d only in the first, %d only in the second" % (len(common), differ, len(only_a), len(only_b)))
    return 1 if differ or only_b else 0


def main():
    bad = 0
    args = sys.argv[1:]
    if args and args[0] == "--exact":
        sys.exit(exact(args[1], args[2]))
    cap = None      # wavefronts per SIMD of the one resident workgroup
    if args and args[0] == "--one-workgroup-per-cu":
        cap = int(args[1]) // 64 // 4
        args = args[2:]
        print("occupancy gated as min(occupancy, %d): one workgroup of %d wavefronts per CU is resident" % (cap, 4 * cap))
    for before, after in zip(args[0::2], args[1::2]):
        a, b = kernels(before), kernels(after)
        print("== %s -> %s: %d / %d kernels" % (before.split("/")[-1], after.split("/")[-1], len(a), len(b)))
        if set(a) != set(b):
            bad += 1
            print("KERNEL SYMBOLS DIFFER: only before %s, only after %s" % (sorted(set(a) - set(b)), sorted(set(b) - set(a))))
        names = sorted(set(a) & set(b))
        demangled = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
        print("%-6s %-9s %-7s %-7s %-9s %-11s %-9s %-10s %-4s kernel" % ("mfma", "lds", "barrier", "glb", "scr", "valu", "vgpr", "scratch B", "occ"))
        worst_valu = 0.0
        for name, dem in zip(names, demangled):
            x, y = a[name], b[name]
            gate = [k for k in ("mfma", "lds", "barrier") if x[k] != y[k]]
            if (x["occ"] != y["occ"]) if cap is None else (min(x["occ"], cap) != min(y["occ"], cap)):
                gate.append("occ")
            if x["glb"] + x["scr"] != y["glb"] + y["scr"] and x["scratch"] == y["scratch"]:
                gate.append("glb+scr at equal scratch bytes")
            bad += bool(gate)
            worst_valu = max(worst_valu, abs(y["valu"] - x["valu"]) / x["valu"])

            def pair(k):
                return "%d" % x[k] if x[k] == y[k] else "%d>%d" % (x[k], y[k])
            short = re.sub(r"\(anonymous namespace\)::|void |\(NfProgram, NfLaunch\)", "", dem)
            print("%-6s %-9s %-7s %-7s %-9s %-11s %-9s %-10s %-4s %s%s" % (pair("mfma"), pair("lds"), pair("barrier"), pair("glb"), pair("scr"), pair("valu"),
                                                                        pair("vgpr"), pair("scratch"), pair("occ"), short,
                                                                        "   <-- GATED: " + ", ".join(gate) if gate else ""))
        print("largest VALU count change: %.1f %%" % (100.0 * worst_valu))
    print("RESULT: %s" % ("%d gated difference(s)" % bad if bad else "every gated class equal"))
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
