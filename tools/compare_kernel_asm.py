#!/usr/bin/env python3
"""Compare the kernel bodies of two `make asm` outputs of one kernel unit (csrc/asm/erpl_k64.s before and after a change
that adds kernels to the unit): every kernel of the first file must be in the second with the same instructions AND the
same kernel descriptor (its .amdhsa_kernel block: registers, scratch, LDS, what the occupancy follows from).  What may
differ is what a kernel's position in the unit decides: the function number in local labels (.LBB5_3 -> .LBB6_3) and the
assembler comments that quote them.  Exit status: the number of kernels that differ or are missing.

    python tools/compare_kernel_asm.py before/erpl_k64.s erpl_monte_carlo_sim_amd/csrc/asm/erpl_k64.s
"""
import re
import sys


def kernels(path):
    text = open(path).read()
    return {m.group(1): m.group(0) for m in re.finditer(r"^(_Z\w+):.*?^\.Lfunc_end\d+:", text, re.S | re.M)}


def descriptors(path):
    text = open(path).read()
    return {m.group(1): [line.split(";")[0].strip() for line in m.group(2).split("\n") if line.split(";")[0].strip()]
            for m in re.finditer(r"^\s*\.amdhsa_kernel\s+(\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M)}


def body(text):
    lines = []
    for line in text.split("\n"):
        line = line.split(";")[0].rstrip()
        if line.strip():
            lines.append(re.sub(r"\.L(BB|func_end|func_begin|tmp|JTI)\d+", r".L\1N", line))
    return lines


def main(before, after):
    a, b = kernels(before), kernels(after)
    da, db = descriptors(before), descriptors(after)
    assert set(da) == set(a), "every kernel has one descriptor"
    bad = 0
    for name, text in a.items():
        same = name in b and body(text) == body(b[name]) and da[name] == db.get(name)
        bad += not same
        print(("same  " if same else "DIFF  ") + name)
    for name in b:
        if name not in a:
            print("new   " + name)
    return bad


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
