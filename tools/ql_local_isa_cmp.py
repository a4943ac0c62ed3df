#!/usr/bin/env python3
"""Developer tool (no GPU needed): do the kernels of a unit have the instruction streams of another revision's?
Compiles csrc/<unit> (steinhardt_local.hip unless given) of <git revision> and of this tree to gfx950 assembly with the Makefile's
flags and compares, kernel by kernel (those whose name holds <prefix>, k_qll unless given): instruction count, identical text, identical
opcode sequence; for a kernel whose sequence differs, whether the histogram of its fp64 opcodes is the other revision's.  With
pair_entropy.hip k_pe and env_similarity.hip k_es it serves the units that share row_walk.hpp (profiles/r20, profiles/r26).  "Text" is
the instruction lines without the kernel's number in its branch targets (.LBB<number>_<block>).
For steinhardt_local.hip: a revision with this tree's kernel names is compared name by
name (all 60 instantiations: profiles/r10/qll_isa_cmp.txt); the 24 kernels of a revision from before the options with the plain
instantiations of this tree (k_qll_accumulate<.., QLL_PLAIN>, k_qll_forces<.., false>, k_qll_forces_tile<.., false>:
profiles/r8/qll_isa_cmp.txt); the force kernels of a revision from before the virial switch with the VIR = false instantiations
(k_qll_forces<.., AVG, false>, k_qll_forces_tile<.., AVG, false>: profiles/r12/qll_isa_cmp.txt).
usage: tools/ql_local_isa_cmp.py <git revision> [<unit>.hip [<kernel-name prefix>]]"""
import os
import re
import subprocess
import sys
import tempfile

root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = "--offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wall -Wno-unused-function -ffp-contract=fast -S --cuda-device-only".split()


def assembly(tree, unit, out):
    csrc = os.path.join(tree, "metadynamics-plugin_amd", "csrc")
    subprocess.check_call([HIPCC] + FLAGS + ["-I" + os.path.join(tree, "include"), "-I" + csrc, os.path.join(csrc, unit), "-o", out])


def kernels(path, prefix):
    """{demangled short name: [instruction lines]} of the <prefix>* kernels of an assembly file"""
    out, cur, name = {}, None, None
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and prefix in m.group(1):
            name, cur = m.group(1), []
            continue
        if cur is None:
            continue
        t = line.strip()
        if t.startswith(".Lfunc_end"):
            out[name] = cur
            cur = None
        elif t and not t.startswith(".") and not t.startswith(";"):
            # (a branch target .LBB<n>_<block> carries the kernel's number in its unit, which moves when a kernel before it comes or goes)
            cur.append(re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"\s*;.*", "", t)))
    names = list(out)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.strip().split("\n")
    short = [re.sub(r"\(anonymous namespace\)::|void |HIP_vector_type<|, 4u>", "", re.sub(r"\(mtd::.*", "", d)) for d in dem]
    return dict(zip(short, out.values()))


def fp64_histogram(body):
    h = {}
    for x in body:
        op = x.split()[0]
        if op.startswith("v_") and "f64" in op:
            h[op] = h.get(op, 0) + 1
    return h


def main(rev, unit="steinhardt_local.hip", prefix="k_qll"):
    with tempfile.TemporaryDirectory() as tmp:
        old_tree = os.path.join(tmp, "old")
        os.mkdir(old_tree)
        tar = subprocess.run(["git", "-C", root, "archive", rev, "metadynamics-plugin_amd/csrc", "include"], capture_output=True, check=True).stdout
        subprocess.run(["tar", "-x", "-C", old_tree], input=tar, check=True)
        assembly(old_tree, unit, os.path.join(tmp, "old.s"))
        assembly(root, unit, os.path.join(tmp, "new.s"))
        old, new = kernels(os.path.join(tmp, "old.s"), prefix), kernels(os.path.join(tmp, "new.s"), prefix)
    same = True
    ops = lambda body: [x.split()[0] for x in body]
    for k, body in sorted(old.items()):
        k2 = k if k in new else k[:-1] + (", 0>" if "accumulate" in k else ", false>")          # the plain / VIR = false instantiation of this tree
        b2 = new.get(k2)
        if b2 is None:
            print("%-40s has no counterpart %s" % (k, k2))
            same = False
            continue
        same = same and ops(body) == ops(b2)
        print("%-40s %5d vs %5d instructions; identical text: %s; identical opcode sequence: %s" % (k, len(body), len(b2), body == b2, ops(body) == ops(b2)))
        if ops(body) != ops(b2):
            print("%-40s fp64 opcode histogram identical: %s" % ("", fp64_histogram(body) == fp64_histogram(b2)))
    return 0 if same else 1


if __name__ == "__main__":
    if not 2 <= len(sys.argv) <= 4:
        sys.exit(__doc__)
    sys.exit(main(*sys.argv[1:]))
