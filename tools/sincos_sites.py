"""The sincosFast stretches inlined in the kernels of a disassembly made by tools/isa_dump.sh: python tools/sincos_sites.py file.s kernel-substring [...]
From each v_rndne_f64 (q = rint(x 2/pi), the first statement of sincosFast) the expression trees of the sine and of the cosine polynomial's result are rebuilt
from the v_fma_f64 / v_fmac_f64 / v_mul_f64 / v_add_f64 that follow, with x, q, the table constants (S) and literals as leaves.  Two inline sites round alike
iff their trees are equal: the same instructions with the same operand roles, whatever the schedule and the register numbers.  sincosFast is compiled with
contraction on, so which products are fused into which sums is the compiler's choice at each site; kernels that must agree bit for bit (uph_footprint_kernel and
uph_footprint_sweep_kernel) need the same choice at every site, and this shows it before a GPU is involved.  Exit status 1 if a site differs from the first."""
import re
import sys


def kernels(path):
    """mangled name -> instruction lines (tools/isa_compare.py's reading of the file)"""
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
    return {k: v for k, v in out.items() if v and not k.endswith(".kd")}


def pair(o):
    m = re.fullmatch(r"([vs])\[(\d+):(\d+)\]", o)
    return (m.group(1), int(m.group(2)), int(m.group(3))) if m else None
def site(ins, at):
    mulsrc = ins[at].split(",")[1].strip()
    x = None
    for j in range(at - 1, max(at - 60, -1), -1):
        p = ins[j].split(None, 1)
        if p[0].startswith("v_mul_f64") and p[1].split(",")[0].strip() == mulsrc:
            x = [o.strip() for o in p[1].split(",")][1:]
            break
    E = {}                                  # vgpr pair -> expression
    for o in x or []:
        if o.startswith("v["):
            E[o] = "x"
    E[ins[at].split()[1].rstrip(",")] = "q"
    def leaf(o):
        neg, o2 = o.startswith("-"), o.lstrip("-")
        ab = o2.startswith("|")
        o2 = o2.strip("|")
        if o2 in E: e = E[o2]
        elif o2.startswith("s["): e = "S"
        elif o2.startswith("v["): e = "V"
        else: e = o2
        return ("-" if neg else "") + ("abs(%s)" % e if ab else e)
    def clobber(dst):
        if dst.startswith("v["):
            p = pair(dst); lo, hi = p[1], p[2]
        elif re.fullmatch(r"v\d+", dst):
            lo = hi = int(dst[1:])
        else:
            return
        for k in list(E):
            kp = pair(k)
            if kp and kp[0] == "v" and not (kp[2] < lo or kp[1] > hi):
                del E[k]
    found = {}
    consts = {}                             # single vgprs loaded from scalars (table constants moved to vector registers)
    for p in ins[at + 1:at + 260]:
        sp = p.split(None, 1)
        if len(sp) < 2: continue
        op, ops = sp[0].replace("_e64", "").replace("_e32", ""), [o.strip() for o in sp[1].split(",")]
        if op in ("v_mul_f64", "v_add_f64", "v_fma_f64", "v_fmac_f64"):
            srcs = [leaf(o) for o in ops[1:]]
            if op == "v_fmac_f64": srcs.append(leaf(ops[0]))
            e = {"v_mul_f64": "mul", "v_add_f64": "add", "v_fma_f64": "fma", "v_fmac_f64": "fma"}[op] + "(" + ",".join(srcs) + ")"
            clobber(ops[0])
            if "x" in e or "q" in e:
                E[ops[0]] = e
                r = "fma(-q,S,fma(-q,S,x))"
                if e.startswith("add(" + r + ",-"): found.setdefault("sin", e)
                if e.startswith("add(fma(mul(%s,%s),-0.5,1.0)," % (r, r)): found.setdefault("cos", e)
        elif op == "v_mov_b32" and ops[1].startswith("s"):
            clobber(ops[0])                 # (a constant: reads as V -> normalised below)
        elif op.startswith(("v_", "ds_read", "global_load", "buffer_load", "flat_load")):
            clobber(ops[0])
        if len(found) == 2: break
    return found
def norm(e):                                # table constants read S from a scalar pair and V once moved to a vector pair: one leaf
    return re.sub(r"\bV\b", "S", e)
if len(sys.argv) < 3:
    sys.exit(__doc__)
K = kernels(sys.argv[1])
ref = None
ok = True
for k, ins in sorted(K.items()):
    if not any(s in k for s in sys.argv[2:]): continue
    for at, i in enumerate(ins):
        if i.startswith("v_rndne_f64"):
            f = site(ins, at)
            f = {n: norm(e) for n, e in f.items()}
            if ref is None:
                ref = f
                print("reference site (%s, instruction %d):\n  sin = %s\n  cos = %s" % (k, at, f.get("sin"), f.get("cos")))
            same = f == ref and len(f) == 2
            ok &= same
            print("%-90s instruction %5d  sin and cos trees found: %d  equal to the reference: %s" % (k[:90], at, len(f), same))
            if not same: print("   ", f)
print("every site rounds as the reference site" if ok and ref else "DIFFERENT (or no site found)")
sys.exit(0 if ok and ref else 1)
