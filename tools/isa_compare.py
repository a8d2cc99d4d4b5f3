"""Per-kernel comparison of two disassemblies made by tools/isa_dump.sh: python tools/isa_compare.py A.s B.s
For every kernel of A: whether B has it instruction for instruction (up to s_endpgm, address comments and symbol operands stripped), and whether it
does once the immediates of the s_add_u32 / s_addc_u32 that follow an s_getpc_b64 are masked (the pc-relative address of a constant table, which
moves when code is added to the code object).  uph_solver_kernel instantiations are counted, every other kernel gets a line.  Kernels are paired by
mangled name; what that leaves over on both sides (a kernel whose argument struct was renamed) is paired by the demangled name before the parameter
list, where that pairs one with one, and its lines say so; then the kernels only one side has."""
import re
import subprocess
import sys


def kernels(path):
    out, name = {}, None
    for line in open(path, errors="ignore"):
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            name = m.group(1)
            out[name] = []
            continue
        if name is None or not line.startswith("\t"):
            continue
        ins = re.sub(r"<[^>]*>", "<sym>", line.split("//")[0].strip())
        if ins:
            out[name].append(ins)
    for k, v in out.items():
        if "s_endpgm" in v:
            out[k] = v[:v.index("s_endpgm") + 1]
    return {k: v for k, v in out.items() if v and not k.endswith(".kd")}


def masked(ins):
    out, since = [], 99
    for i in ins:
        since = 0 if i.startswith("s_getpc_b64") else since + 1
        if since <= 6 and re.match(r"s_addc?_u32 ", i):
            i = re.sub(r",\s*(0x[0-9a-f]+|-?\d+)$", ", <pcrel>", i)
        out.append(i)
    return out


def before_params(names):
    """mangled -> the demangled name up to its parameter list: `void uph_extent_kernel<256>`"""
    names = sorted(names)
    if not names:
        return {}
    try:
        dem = subprocess.run(["c++filt"] + names, stdin=subprocess.DEVNULL, capture_output=True, text=True, check=True).stdout.split("\n")[:len(names)]
    except (OSError, subprocess.CalledProcessError):      # no demangler: nothing is paired
        dem = names
    out = {}
    for n, d in zip(names, dem):
        depth, cut = 0, len(d)
        for i, ch in enumerate(d):
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0:
                cut = i
                break
        out[n] = d[:cut]
    return out


def line(k, x, y, note=""):
    print("%-100s %5d instructions  identical: %s  (pc-relative offsets aside: %s)%s" % (k[:100], len(x), x == y, masked(x) == masked(y), note))


a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
sol = [k for k in a if "uph_solver_kernel" in k]
print("uph_solver_kernel instantiations: %d, in both: %d, ISA identical (pc-relative constant offsets aside): %d, byte-identical: %d" % (
    len(sol), sum(k in b for k in sol), sum(k in b and masked(a[k]) == masked(b[k]) for k in sol), sum(k in b and a[k] == b[k] for k in sol)))
for k in sorted(a):
    if k in b and "uph_solver_kernel" not in k:
        line(k, a[k], b[k])
# the leftovers, by the name before the parameter list
na, nb = before_params(k for k in a if k not in b), before_params(k for k in b if k not in a)
for k, short in sorted(na.items()):
    other = [j for j, s in nb.items() if s == short]
    if sum(s == short for s in na.values()) == 1 and len(other) == 1:
        line(short, a.pop(k), b.pop(other[0]), "  [paired by name: the parameter types differ]")
print("only in %s: %s" % (sys.argv[1], sorted(k for k in a if k not in b)))
print("only in %s: %s" % (sys.argv[2], sorted(k for k in b if k not in a)))
