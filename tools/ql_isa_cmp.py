#!/usr/bin/env python3
"""Developer tool (no GPU needed): do the kernels of steinhardt.hip have the instruction streams of another revision's, and what do
they cost?  Compiles csrc/steinhardt.hip of <git revision> and of this tree to gfx950 assembly with the Makefile's flags and compares,
kernel by kernel: instruction count, identical text, identical opcode sequence.  A kernel of a revision from before the virial switch is
compared with the VIR = false instantiation of this tree (k_ql_forces<.., CARRY, false>: profiles/r13/ql_isa_cmp.txt).  Then the
compiler's resource usage (-Rpass-analysis=kernel-resource-usage) of every k_ql_forces instantiation of both, side by side, and of the
VIR kernels beside the plain full-list kernel of the same array type and LMAX (profiles/r13/ql_resource_usage.txt).
usage: tools/ql_isa_cmp.py <git revision>"""
import os
import re
import subprocess
import sys
import tempfile

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = ("--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -ffp-contract=fast -S --cuda-device-only "
         "-Rpass-analysis=kernel-resource-usage").split()
FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]


def short_names(mangled):
    dem = subprocess.run(["c++filt"] + mangled, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    return [re.sub(r"\(anonymous namespace\)::|void |HIP_vector_type<|, 4u>", "", re.sub(r"\(mtd::.*", "", d)) for d in dem]


def assembly(tree, out):
    """compiles the unit; returns {mangled name: {field: value}} from the compiler's remarks"""
    csrc = os.path.join(tree, "metadynamics-plugin_amd", "csrc")
    err = subprocess.run([HIPCC] + FLAGS + ["-I" + os.path.join(tree, "include"), "-I" + csrc, os.path.join(csrc, "steinhardt.hip"), "-o", out],
                         capture_output=True, text=True, check=True).stderr
    usage, cur = {}, None
    for line in err.split("\n"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = usage.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    return usage


def kernels(path):
    """{demangled short name: [instruction lines]} of the k_ql_* kernels of an assembly file"""
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and "k_ql_" in m.group(1):
            name, cur = m.group(1), []
            continue
        if cur is None:
            continue
        t = line.strip()
        if t.startswith(".Lfunc_end"):
            out[name] = cur
            cur = None
        elif t and not t.startswith(".") and not t.startswith(";"):
            cur.append(re.sub(r"\s*;.*", "", t))
    return dict(zip(short_names(list(out)), out.values()))


def by_short_name(usage):
    names = [n for n in usage if "k_ql_" in n]
    return dict(zip(short_names(names), [usage[n] for n in names]))


def main(rev):
    with tempfile.TemporaryDirectory() as tmp:
        old_tree = os.path.join(tmp, "old")
        os.mkdir(old_tree)
        tar = subprocess.run(["git", "-C", root, "archive", rev, "metadynamics-plugin_amd/csrc", "include"], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", old_tree], input=tar, check=True)
        old_use = by_short_name(assembly(old_tree, os.path.join(tmp, "old.s")))
        new_use = by_short_name(assembly(root, os.path.join(tmp, "new.s")))
        old, new = kernels(os.path.join(tmp, "old.s")), kernels(os.path.join(tmp, "new.s"))
    same = True
    ops = lambda body: [x.split()[0] for x in body]
    counterpart = lambda k: k if k in new else k[:-1] + ", false>"          # the VIR = false instantiation of this tree
    print("== instruction streams: %s against this tree ==" % rev)
    for k, body in sorted(old.items()):
        k2 = counterpart(k)
        b2 = new.get(k2)
        if b2 is None:
            print("%-50s has no counterpart %s" % (k, k2))
            same = False
            continue
        same = same and ops(body) == ops(b2)
        print("%-50s %5d vs %5d instructions; identical text: %s; identical opcode sequence: %s" % (k, len(body), len(b2), body == b2, ops(body) == ops(b2)))
    row = lambda u: "  ".join("%6s" % u.get(f, "?") for f in FIELDS)
    print("\n== resource usage: %s | this tree ==" % rev)
    print("%-50s %s" % ("columns (twice):", " / ".join(FIELDS)))
    for k in sorted(old):
        if k in old_use and counterpart(k) in new_use:
            equal = all(old_use[k].get(f) == new_use[counterpart(k)].get(f) for f in FIELDS)
            same = same and equal
            print("%-50s %s | %s  %s" % (k, row(old_use[k]), row(new_use[counterpart(k)]), "same" if equal else "DIFFERENT"))
    print("\n== the VIR kernels of this tree, each under the plain full-list kernel of its array type and LMAX ==")
    for k in sorted(new):
        if k.startswith("k_ql_forces<") and k.endswith(", false, false, false, true>"):
            plain = k[:-len("true>")] + "false>"
            print("%-50s %s" % (plain, row(new_use[plain])))
            print("%-50s %s" % (k, row(new_use[k])))
    return 0 if same else 1


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1]))
