#!/usr/bin/env python3
"""tools/loads_in_flight.py <file.s> -- for every moe_combine_rmsnorm_kernel of a hipcc -S device assembly of csrc/rmsnorm_quant.hip: the largest number
of 16-byte global loads outstanding at a wait that retires one, against the kernel's group of slot loads (slots per group x columns per thread).

A straight-line reading of the text: the count of outstanding loads starts at 0 at every label, rises by one per global_load_dwordx4, and an
`s_waitcnt vmcnt(k)` with k below the count retires loads down to k (a wait with k at or above it retires none).  The vector-memory counter is in
order, so the largest count met at a retiring wait is the number of loads the kernel really has in flight together.  Exit status 1 when a kernel
falls short of its group."""
import re
import sys

res, name, out = {}, None, 0
for line in open(sys.argv[1]):
    m = re.match(r"^(_Z\w*moe_combine_rmsnorm_kernel\w+):", line)
    if m:
        name, out = m.group(1), 0
        res[name] = [0]
        continue
    if name is None:
        continue
    l = line.strip()
    if l.startswith(".Lfunc_end"):
        name = None
    elif l.startswith(".LBB"):
        out = 0
    elif l.startswith("global_load_dwordx4"):
        out += 1
    elif l.startswith("s_waitcnt"):
        m = re.search(r"vmcnt\((\d+)\)", l)
        if m and int(m.group(1)) < out:
            res[name].append(out)
            out = int(m.group(1))
short = 0
for k, v in res.items():
    bf, act, ilp = map(int, re.search(r"ILb(\d)ELi(\d)ELi(\d)E", k).groups())
    depth = 2 if ilp >= 4 else 8 // ilp
    good = max(v) >= depth * ilp
    short += not good
    print(f"{'bf16' if bf else 'fp16'} format {act} columns {ilp}: group {depth} x {ilp} = {depth * ilp:2d} loads, outstanding at a retiring wait: {max(v):2d}"
          + ("" if good else "  SHORT"))
print(f"{len(res)} kernels, {short} short of their group")
sys.exit(1 if short else 0)
