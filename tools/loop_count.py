"""Static instruction counts, by class, of the lane-private cluster loop (scan.h flat_leaf_step, the
`if (!deal)` loop) of one render_kernel instantiation in `make -C atray_amd/csrc asm` output, next to the
whole kernel's. The loop is found in the listing, not by name: the smallest backward-branch interval
that holds the kernel's first v_dot2_f32_f16 (the screen of cluster_cands; the lane-private loop comes
before the dealt rounds), extended over every loop that starts inside it (the blocks the compiler lays
out behind the first back edge).

    python tools/loop_count.py atray_amd/_lib/asm/render.s [ILi7ELb0ELb1ELi7ELb0ELb1E]

The second argument is the template-argument part of the mangled name; the default is the 7-wave
primary table kernel, render_kernel<HYBRID, false, true, 7, false, true>."""
import re
import sys

path = sys.argv[1]
key = sys.argv[2] if len(sys.argv) > 2 else "ILi7ELb0ELb1ELi7ELb0ELb1E"
lines = open(path).read().split("\n")
start = next(i for i, l in enumerate(lines) if re.match(r"^_ZN3atr13render_kernel" + key + r".*:", l))
end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
body = lines[start:end + 1]
labels = {m.group(1): i for i, l in enumerate(body) if (m := re.match(r"^(\.LBB\d+_\d+):", l))}
loops = []
for i, l in enumerate(body):
    m = re.match(r"\s+s_c?branch\w*\s+(\.LBB\d+_\d+)", l)
    if m and m.group(1) in labels and labels[m.group(1)] < i:
        loops.append((labels[m.group(1)], i))
dots = [i for i, l in enumerate(body) if "v_dot2_f32_f16" in l]
a, b = min(((x, y) for x, y in loops if x <= dots[0] <= y), key=lambda xy: xy[1] - xy[0])
grown = True
while grown:
    grown = False
    for x, y in loops:
        if a < x <= b and y > b:
            b, grown = y, True


def classify(rng):
    c = dict.fromkeys(["valu", "v_mov", "v_rcp", "dpp", "s_nop", "salu", "lds", "vmem", "smem", "other", "total"], 0)
    for l in rng:
        s = l.strip()
        if not s or s.startswith(";") or s.startswith(".") or re.match(r"^[\w.$]+:", s):
            continue
        op = s.split()[0]
        c["total"] += 1
        if op.startswith("v_"):
            c["valu"] += 1
            c["v_mov"] += op.startswith("v_mov_b32")
            c["v_rcp"] += op.startswith("v_rcp")
            c["dpp"] += "row_shr" in s or "row_bcast" in s
        elif op == "s_nop":
            c["s_nop"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith(("global_", "flat_", "buffer_", "scratch_")):
            c["vmem"] += 1
        elif op.startswith(("s_load", "s_buffer_load")):
            c["smem"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
        else:
            c["other"] += 1
    return c


print("loop: listing lines %d..%d of the kernel's %d, %d of its %d screen dots" %
      (a, b, len(body), sum(1 for d in dots if a <= d <= b), len(dots)))
print("loop  ", classify(body[a:b + 1]))
print("kernel", classify(body))
