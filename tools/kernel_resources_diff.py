"""Parent-against-new table of every kernel of `hipcc -S` listings: VGPRs, AGPRs, SGPRs, scratch bytes, static LDS, wave occupancy (the
listing's "Kernel info" comments — the figures of the code-object notes tools/check_no_scratch.py reads) and the instruction mix of
the MFMA loop (as tools/isa_loop.py, but the loop is taken from the listing's loop annotations, so block placement does not move it).  Kernels are paired by demangled name; --drop removes text from the parent's names
first (a template parameter that went away): --drop "gemm_panel_kernel:, 1, " replaces the first ", 1, " by ", " in that kernel's names;
--rename rewrites them by a regular expression (kernels that were folded onto another's name): --rename "old_kernel<(.*)>=new_kernel<\\1, Policy>".
usage: python tools/kernel_resources_diff.py parent_dir new_dir file.s [file.s ...] [--drop KERNEL:TEXT ...] [--rename REGEX=REPL ...]"""
import re, subprocess, sys
from collections import Counter

FIELDS = [("vgpr", r"; NumVgprs: (\d+)"), ("agpr", r"; NumAgprs: (\d+)"), ("sgpr", r"; TotalNumSgprs: (\d+)"), ("scratch", r"; ScratchSize: (\d+)"),
          ("lds", r"; LDSByteSize: (\d+)"), ("occ", r"; Occupancy: (\d+)")]


def loop_mix(lines):
    """the natural loop with the fewest instructions among those that hold MFMAs, by the listing's own loop annotations (a block
    belongs to the loop whose header its label comment names, and to that loop's parents)"""
    loops, cur = {}, []
    for k, l in enumerate(lines):
        m = re.match(r'^\.L(BB\d+_\d+):(.*)$', l)
        if m:
            cur = re.findall(r'Header=(BB\d+_\d+)', m.group(2)) + ([m.group(1)] if 'Loop Header' in m.group(2) else [])
            k2 = k + 1
            while k2 < len(lines) and lines[k2].startswith(';'):                      # "Parent Loop BBx_y Depth=d" lines
                cur += re.findall(r'Parent Loop (BB\d+_\d+)', lines[k2])
                k2 += 1
        elif l.startswith("\t") and l.split() and not l.split()[0].startswith((".", ";")):
            for h in cur:
                loops.setdefault(h, []).append(l.split()[0])
    best = None
    for h, ops in loops.items():
        if any('v_mfma' in o for o in ops) and (best is None or len(ops) < len(best)):
            best = ops
    if best is None:
        return "no MFMA loop"
    ops = Counter(best)
    return "%d instr: " % sum(ops.values()) + " ".join("%s=%d" % kv for kv in sorted(ops.items()))


def kernels(path, drops, renames=()):
    s = open(path).read()
    out = {}
    for m in re.finditer(r'^(_Z\w+):.*?^; Kernel info:(.*?)^; Occupancy: \d+', s, re.M | re.S):
        name, body = m.group(1), m.group(0)
        if ".amdhsa_kernel " + name not in s:
            continue
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        dem = re.sub(r'\((?!anonymous namespace\)$)(?:[^()]|\(anonymous namespace\))*\)$', '', dem)     # the parameter list
        for d in drops:
            kernel, text = d.split(":", 1)
            if kernel in dem:
                dem = dem.replace(text, ", ", 1)
        for r in renames:
            dem = re.sub(*r.split("=", 1), dem)
        res = {k: int(re.search(p, body).group(1)) for k, p in FIELDS}
        res["loop"] = loop_mix(body[:body.index("; Kernel info:")].splitlines())
        out[dem] = res
    return out


def main():
    args, drops, renames = [], [], []
    it = iter(sys.argv[1:])
    for a in it:
        if a == "--drop":
            drops.append(next(it))
        elif a == "--rename":
            renames.append(next(it))
        else:
            args.append(a)
    pdir, ndir, files = args[0], args[1], args[2:]
    ndiff = 0
    for f in files:
        a, b = kernels("%s/%s" % (pdir, f), drops, renames), kernels("%s/%s" % (ndir, f), [])
        print("== %s: %d kernels (parent), %d (new)" % (f, len(a), len(b)))
        for name in sorted(set(a) | set(b)):
            x, y = a.get(name), b.get(name)
            if x is None or y is None:
                print("  %s: only in %s" % (name, "new" if x is None else "parent")); ndiff += 1; continue
            same = x == y
            ndiff += not same
            print("  %s\n    vgpr %d agpr %d sgpr %d scratch %d lds %d occupancy %d | loop %s%s" % (
                name, y["vgpr"], y["agpr"], y["sgpr"], y["scratch"], y["lds"], y["occ"], y["loop"], "  [= parent]" if same else ""))
            if not same:
                print("    PARENT: vgpr %d agpr %d sgpr %d scratch %d lds %d occupancy %d | loop %s" % (
                    x["vgpr"], x["agpr"], x["sgpr"], x["scratch"], x["lds"], x["occ"], x["loop"]))
    print("kernels that differ from the parent: %d" % ndiff)


main()
