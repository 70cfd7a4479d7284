#!/usr/bin/env python3
"""Compare the device code of two source trees kernel by kernel.

    hipcc <the Makefile's FLAGS> --cuda-device-only -S x.hip -o OLD/x.s     (and NEW/x.s)
    python tools/kernel_asm_diff.py OLD NEW

Per kernel symbol: identical = the same instruction text (comments stripped) and resource lines;
equivalent = the same resources and the same opcodes as often, differing in registers or order;
changed = anything else.  Prints a tally per file and every kernel that is not identical."""
import collections
import os
import re
import sys

RES = re.compile(r"; (TotalNumSgprs|NumVgprs|NumAgprs|ScratchSize|Occupancy|LDSByteSize): *(\S+)")


def kernels(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            cur = out[m.group(1)] = ([], {})
            continue
        if cur is None:
            continue
        r = RES.search(line)
        if r:
            cur[1][r.group(1)] = r.group(2)
        code = re.sub(r"\.L(BB|func_end|func_begin)\d+", r".L\1", line.split(";")[0]).strip()
        if code and not code.startswith(".") and not code.endswith(":") and not cur[1]:
            cur[0].append(code)
    return out


def main(old_dir, new_dir):
    for name in sorted(os.listdir(old_dir)):
        old, new = kernels(os.path.join(old_dir, name)), kernels(os.path.join(new_dir, name))
        tally = collections.Counter()
        for k in sorted(set(old) | set(new)):
            if k not in old or k not in new:
                cls = "only in " + ("old" if k in old else "new")
            elif old[k] == new[k]:
                cls = "identical"
            elif old[k][1] == new[k][1] and collections.Counter(i.split()[0] for i in old[k][0]) == \
                    collections.Counter(i.split()[0] for i in new[k][0]):
                cls = "equivalent"
            else:
                cls = "changed"
            tally[cls] += 1
            if cls != "identical":
                o, n = old.get(k, ([], {})), new.get(k, ([], {}))
                print(f"  {cls}: {k}  instructions {len(o[0])} -> {len(n[0])}  {o[1]} -> {n[1]}")
        print(f"{name}: {dict(tally)}")


if __name__ == "__main__":
    main(*sys.argv[1:3])
