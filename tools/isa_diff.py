#!/usr/bin/env python3
"""tools/isa_diff.py <old.s> <new.s> [filter] -- compare two `hipcc -S --cuda-device-only` outputs kernel by kernel.

For each kernel present in both files: the instruction count of each side, whether the instruction streams are identical (operands
included; block labels are compared by position, not by number), whether at least the opcode sequences are, and otherwise the opcodes whose
counts differ, as (old, new).  An operand written name(number) counts into the opcode: `s_waitcnt vmcnt(3)` is `s_waitcnt vmcnt`."""
import collections
import re
import sys


def kernels(path):
    """name -> list of instruction texts for every .amdhsa_kernel of the file"""
    text = open(path).read()
    names = set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))
    out, cur, labels = {}, None, {}
    for line in text.split("\n"):
        m = re.match(r"^([A-Za-z_.$][\w.$]*):", line)
        if m:
            if m.group(1) in names:
                cur, labels = out.setdefault(m.group(1), []), {}
            elif m.group(1).startswith(".Lfunc_end"):
                cur = None
            elif cur is not None:
                labels[m.group(1)] = len(labels) + 1
            continue
        if cur is None or not line.startswith("\t"):
            continue
        ins = line.split(";")[0].strip()
        if ins and not ins.startswith("."):
            cur.append((" ".join(ins.split()), labels))
    # a branch target is named by its block's ordinal within the kernel
    return {k: [re.sub(r"\.LBB\d+_\d+", lambda t: "L%s" % lab.get(t.group(0), "?"), i) for i, lab in v] for k, v in out.items()}


def opcode(ins):
    return " ".join([ins.split()[0]] + re.findall(r"\b([a-z_]+)\(\d+\)", ins))


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    flt = sys.argv[3] if len(sys.argv) > 3 else ""
    for name in old:
        if name not in new or flt not in name:
            continue
        a, b = old[name], new[name]
        ops_a, ops_b = [opcode(i) for i in a], [opcode(i) for i in b]
        short = re.sub(r"^_ZN9petit_amd\d+", "", name)[:110]
        verdict = "identical" if a == b else "same opcode sequence" if ops_a == ops_b else "differ"
        print(f"old {len(a):6d} new {len(b):6d}  {verdict:20s}  {short}")
        if ops_a != ops_b:
            ca, cb = collections.Counter(ops_a), collections.Counter(ops_b)
            print("    " + "  ".join(f"{op} ({ca[op]}, {cb[op]})" for op in sorted(set(ca) | set(cb)) if ca[op] != cb[op]))
    for name in sorted(set(old) ^ set(new)):
        if flt in name:
            print(f"only in {'old' if name in old else 'new'}: {name}")


if __name__ == "__main__":
    main()
