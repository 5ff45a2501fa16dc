#!/usr/bin/env python3
"""Compare the generated device code of two builds kernel by kernel (no GPU needed).

Both trees are compiled with the Makefile's flags plus `-Rpass-analysis=kernel-resource-usage -save-temps`, one directory of temporaries
each (the `<stem>-hip-amdgcn-amd-amdhsa-gfx950.s` files are read).  For every kernel: VGPRs, AGPRs, SGPRs, scratch, static LDS (the figures
the compiler prints behind the kernel), the instruction count, the count of every `v_mfma_*` and floating-point VALU opcode, and whether the
instruction text equals the other build's with labels, symbol names and comments set aside.  Kernels are matched by demangled name.
The dynamic LDS of a launch is computed by host code and is not in the assembly: compare the host functions that size it.

    python tools/kernel_asm_diff.py PARENT_TEMPS NEW_TEMPS stem [stem ...] > resources.md

Exit status 1 if a hard condition fails: scratch appears, or an MFMA / floating-point opcode count differs.
"""
import collections
import re
import subprocess
import sys

FP = re.compile(r"^v_(mfma|pk_)?(add|sub|mul|fma|fmac|mac|mad|max|min|rcp|rsq|sqrt|div_\w+|cvt|exp|log|ldexp|trunc|floor|ceil|rndne|fract|cndmask)?\w*_(f16|f32|f64|bf16)\b")
FIGS = (("TotalNumSgprs", "SGPR"), ("NumVgprs", "VGPR"), ("NumAgprs", "AGPR"), ("ScratchSize", "scratch"), ("LDSByteSize", "LDS"))


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout
    return dict(zip(names, out.split("\n")))


def key_of(name):
    """the demangled kernel name without namespace, return type and argument list"""
    n = name.replace("(anonymous namespace)::", "")
    n = re.sub(r"^void ", "", n)
    return re.sub(r"\(.*$", "", n)


def kernels(path):
    """{mangled name: (figures, [normalised instruction lines])} of the kernels (symbols with a .amdhsa_kernel descriptor) of a .s file"""
    lines = open(path).read().split("\n")
    kd = {m.group(1) for m in (re.match(r"\s*\.amdhsa_kernel\s+(\S+)", l) for l in lines) if m}
    out, cur, body = {}, None, []
    figs = {}
    for l in lines:
        m = re.match(r"^([A-Za-z_][\w$.]*):", l)
        if m and m.group(1) in kd and cur is None:
            cur, body, figs = m.group(1), [], {}
            continue
        if cur is None:
            continue
        if l.startswith(".Lfunc_end"):
            continue
        m = re.match(r"^; (\w+): (\d+)", l)
        if m and m.group(1) in dict(FIGS):
            figs[dict(FIGS)[m.group(1)]] = int(m.group(2))
            if m.group(1) == "LDSByteSize":
                out[cur] = (figs, body)
                cur = None
            continue
        t = l.split(";")[0].strip()
        if not t or t.startswith(".") and not t.startswith(".LBB"):
            continue
        body.append(t)
    return out


def normalise(body):
    labels = {}
    res = []
    for t in body:
        def lab(m):
            return labels.setdefault(m.group(0), "L%d" % len(labels))
        t = re.sub(r"\.LBB\d+_\d+", lab, t)
        t = re.sub(r"_Z[\w$.]+", "SYM", t)
        res.append(re.sub(r"\s+", " ", t))
    return res


def fp_counts(body):
    c = collections.Counter()
    for t in body:
        op = re.sub(r"_(e32|e64|dpp|sdwa)$", "", t.split(" ")[0])
        if op.startswith("v_mfma") or FP.match(op):
            c[op] += 1
    return c


def opcodes(body):
    return collections.Counter(re.sub(r"_(e32|e64|dpp|sdwa)$", "", t.split(" ")[0]) for t in body if not t.endswith(":"))


def main():
    parent, new, stems = sys.argv[1], sys.argv[2], sys.argv[3:]
    bad = 0
    total = same = 0
    rows, moved = [], []
    for stem in stems:
        sides = []
        for d in (parent, new):
            ks = kernels("%s/%s-hip-amdgcn-amd-amdhsa-gfx950.s" % (d, stem))
            dm = demangle(list(ks))
            sides.append({key_of(dm[k]): v for k, v in ks.items()})
        p, n = sides
        for k in sorted(set(p) | set(n)):
            total += 1
            if k not in p or k not in n:
                rows.append("| `%s.o` | `%s` | %s | | | | | | |" % (stem, k, "only in the parent" if k in p else "only in this tree"))
                bad += 1
                continue
            (pf, pb), (nf, nb) = p[k], n[k]
            pn, nn = normalise(pb), normalise(nb)
            ident = pn == nn and pf == nf
            same += ident
            note = "identical" if ident else "differs"
            pc, nc = fp_counts(pn), fp_counts(nn)
            if pc != nc:
                note += "; FP counts: " + ", ".join("%s %d -> %d" % (o, pc[o], nc[o]) for o in sorted(set(pc) | set(nc)) if pc[o] != nc[o])
                bad += 1
            if nf["scratch"] != 0 and pf["scratch"] == 0:
                note += "; SCRATCH APPEARS"
                bad += 1
            if not ident:
                po, no = opcodes(pn), opcodes(nn)
                d = sorted(((no[o] - po[o], o) for o in set(po) | set(no) if po[o] != no[o]), key=lambda x: (-abs(x[0]), x[1]))
                note += "; opcode counts: " + (", ".join("%s %+d" % (o, n_) for n_, o in d[:6]) + (" ..." if len(d) > 6 else "") if d
                                               else "equal (order / registers only)")
                moved.append((stem, k))
            rows.append("| `%s.o` | `%s` | %d / %d | %d / %d | %d / %d | %d / %d | %d / %d | %d / %d | %s |" % (
                stem, k, len(pn), len(nn), pf["VGPR"], nf["VGPR"], pf["AGPR"], nf["AGPR"], pf["SGPR"], nf["SGPR"], pf["scratch"], nf["scratch"],
                pf["LDS"], nf["LDS"], note))
    print("%d kernels compared, %d identical (instruction text and every resource figure), %d not; hard conditions failed: %d\n" % (
        total, same, total - same, bad))
    print("\n| object | kernel | instructions parent / new | VGPR | AGPR | SGPR | scratch | static LDS | |")
    print("|---|---|---|---|---|---|---|---|---|")
    print("\n".join(rows))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
