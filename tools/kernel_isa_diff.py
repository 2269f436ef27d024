"""Compare two gfx950 assembly files (hipcc --save-temps: *-hip-amdgcn-amd-amdhsa-gfx950.s) kernel by kernel.

    python tools/kernel_isa_diff.py OLD.s NEW.s [--rename REGEX REPL]... [-v]

Kernels are keyed by their mangled symbol; each --rename rewrites the OLD symbols first (for a kernel whose template parameter
list changed: the mangled name spells the list out).  Per kernel the instruction stream and the .amdhsa_* descriptor block are
compared as text: comments and .file / .ident / .loc lines dropped, local labels (.LBB<n>_<m>: <n> counts the file's
functions) and the kernel's own symbol normalised.  Prints the kernels that differ, those only in one file, and the counts;
exit status 1 if anything differs.
"""
import re
import sys


def kernels(path):
    """{symbol: [normalised lines of its body and of its .amdhsa_kernel block]}"""
    lines = open(path).read().split("\n")
    names = [m.group(1) for l in lines if (m := re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l))]
    out = {n: [] for n in names}
    cur = None
    for l in lines:
        l = re.sub(r"\s*(;|//).*$", "", l).rstrip()
        if not l.strip() or re.match(r"\s*\.(file|ident|loc)\b", l):
            continue
        m = re.match(r"(\S+):$", l)
        if m and m.group(1) in out:
            cur = m.group(1)                                  # the kernel's entry label: its body runs to .Lfunc_end
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l)
        if m:
            cur = m.group(1)
        if cur is None:
            continue
        out[cur].append(re.sub(r"\.L(BB|func_end|func_begin|tmp)\d+", r".L\1#", l).replace(cur, "<kernel>"))
        if re.match(r"\s*\.Lfunc_end\d+:", l) or re.match(r"\s*\.end_amdhsa_kernel", l):
            cur = None
    return out


def main(argv):
    verbose = "-v" in argv
    argv = [a for a in argv if a != "-v"]
    ren = []
    while "--rename" in argv:
        i = argv.index("--rename")
        ren.append((argv[i + 1], argv[i + 2]))
        del argv[i:i + 3]
    old, new = kernels(argv[0]), kernels(argv[1])
    for pat, repl in ren:
        old = {re.sub(pat, repl, k): v for k, v in old.items()}
    differ = [k for k in old if k in new and old[k] != new[k]]
    only_old, only_new = [k for k in old if k not in new], [k for k in new if k not in old]
    for k in differ:
        print("DIFFERS   %s  (%d -> %d lines)" % (k, len(old[k]), len(new[k])))
        if verbose:
            import difflib
            print("\n".join(list(difflib.unified_diff(old[k], new[k], lineterm="", n=1))[:80]))
    for k in only_old:
        print("ONLY OLD  %s" % k)
    for k in only_new:
        print("ONLY NEW  %s" % k)
    print("%d kernels in OLD, %d in NEW: %d identical, %d differ, %d only in OLD, %d only in NEW"
          % (len(old), len(new), len([k for k in old if k in new]) - len(differ), len(differ), len(only_old), len(only_new)))
    return 1 if differ or only_old or only_new else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
