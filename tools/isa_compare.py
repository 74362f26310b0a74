#!/usr/bin/env python3
"""Did an edit change any kernel?  Compares two `hipcc -S` device listings function by function.
    hipcc <the Makefile's CXXFLAGS> -S --cuda-device-only -o before.s tracker_kernels.hip     (or any other kernel file of csrc/)
    ... edit ...
    hipcc <the same flags> -S --cuda-device-only -o after.s tracker_kernels.hip
    python tools/isa_compare.py before.s after.s
Prints SAME or DIFF per function symbol (matched by name: the order of the instantiations may change) and, where they differ,
both sides' registers, scratch, LDS, occupancy and code length.  Exit status 1 on any DIFF or on a symbol only one side has.
The text compared is the function's labels and instructions, without comments and without the function's number in local labels."""
import re
import sys

KEYS = ("next_free_vgpr", "next_free_sgpr", "private_segment_fixed_size", "group_segment_fixed_size", "Occupancy", "codeLenInByte")


def functions(path):
    """{symbol: (text lines, {key: value})}; the numbers are the first of each key between this function's start and the next one's"""
    out, sym, in_body = {}, None, False
    for line in open(path):
        m = re.match(r"\s+\.type\s+(\S+),@function", line)
        if m:
            sym, in_body = m.group(1), False
            out[sym] = ([], {})
        if sym is None:
            continue
        text, nums = out[sym]
        m = re.match(r"\s*(?:\.amdhsa_|; )(\w+)(?: = |: | )(\d+)\s*$", line)
        if m and m.group(1) in KEYS:
            nums.setdefault(m.group(1), m.group(2))
        if line.startswith(".Lfunc_end"):
            in_body = False
        code = line.split(";")[0].rstrip()
        if in_body and code:
            text.append(re.sub(r"\.L([A-Za-z]+)\d+_", r".L\1_", code))
        if line.startswith(sym + ":"):
            in_body = True
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    bad = 0
    for sym in sorted(set(a) | set(b)):
        if sym not in a or sym not in b:
            print(f"ONLY IN {sys.argv[1] if sym in a else sys.argv[2]}  {sym}")
            bad += 1
        elif a[sym] == b[sym]:
            print(f"SAME  {sym}")
        else:
            na, nb = a[sym][1], b[sym][1]
            diff = [f"{k} {na.get(k)} -> {nb.get(k)}" for k in KEYS if na.get(k) != nb.get(k)]
            print(f"DIFF  {sym}\n      {', '.join(diff) or 'same registers, scratch, LDS, occupancy and code length'}")
            bad += 1
    print(f"{len(set(a) | set(b))} symbols, {bad} differ or are missing on one side")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
