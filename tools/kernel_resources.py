"""(VGPRs, SGPRs, scratch bytes, LDS bytes, spilled dwords) of every kernel of render.s, paths.s and
guides.s in two `make -C atray_amd/csrc asm` output directories, side by side, with the kernels that differ
marked (a file one directory lacks counts as empty): the table a change to the kernels commits as
profiles/rNN/kernel_resources.txt.

    python tools/kernel_resources.py PARENT_ASM_DIR THIS_ASM_DIR > profiles/rNN/kernel_resources.txt"""
import os
import re
import subprocess
import sys


def table(path):
    out = {}
    if not os.path.exists(path):
        return out
    for blk in open(path).read().split("- .agpr_count:")[1:]:
        def g(k):
            m = re.search(r"\." + k + r":\s+(\S+)", blk)
            return m.group(1) if m else "?"
        out[g("name")] = "(%s, %s, %s, %s, %s)" % (g("vgpr_count"), g("sgpr_count"), g("private_segment_fixed_size"),
                                                   g("group_segment_fixed_size"), g("vgpr_spill_count"))
    return out


pa, ch = sys.argv[1], sys.argv[2]
for f in ["render.s", "paths.s", "guides.s"]:
    print("# " + f)
    a, b = table(pa + "/" + f), table(ch + "/" + f)
    names = list(b)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    for n, d in zip(names, dem):
        x, y = a.get(n, "-"), b[n]
        print(d, x, y, "" if x == y else ("  <-- new" if x == "-" else "  <-- changed"))
