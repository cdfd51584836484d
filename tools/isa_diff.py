#!/usr/bin/env python3
"""Compare two `hipcc -S` outputs (files, or directories of *.s matched by name) kernel by kernel.

    python tools/isa_diff.py OLD NEW [--rename REGEX=REPLACEMENT ...] [--common]

--rename rewrites the names of NEW's kernels (re.sub, in the order given) before they are matched with OLD's: for a kernel whose
code is meant to be the same but whose mangled name moved, e.g. a template that gained a defaulted argument.
--common compares the kernels both sides have and only lists the others: for a change that adds kernels and must leave the
existing ones alone.

Per kernel: VGPR / AGPR / SGPR counts, scratch and LDS bytes, and every opcode whose count differs.  Exit status 1 when a
resource differs, a kernel is missing, or an opcode outside the scalar ALU differs in count; scalar-ALU differences (s_*
arithmetic on registers: moves, adds, shifts, compares) and the scalar no-op the scheduler pads hazards with are listed only.
The classes are read off the operands, not off a list of opcodes: a scalar opcode counts as ALU when it takes a register
operand and moves no dwords, so a jump through a register pair (a call; inlined kernels have none) would be listed, not gated."""
import collections
import os
import re
import sys

RESOURCES = (("vgpr", ".vgpr_count"), ("agpr", ".agpr_count"), ("sgpr", ".sgpr_count"),
             ("scratch", ".private_segment_fixed_size"), ("lds", ".group_segment_fixed_size"))
# a scalar opcode is plain ALU when it computes on registers: not a memory access (those move dwords) and not one of the
# operand-less or immediate-only ones (waits, barriers, branches to a label, end of program)
REGISTER = re.compile(r"\b(?:[sva]\d+\b|[sva]\[\d+:\d+\]|vcc|exec|scc\b|m0\b|flat_scratch)")
PADDING = "s_nop"      # hazard padding: its count follows the instruction order, which is free to differ


def kernels(path):
    files = sorted(os.path.join(path, f) for f in os.listdir(path) if f.endswith(".s")) if os.path.isdir(path) else [path]
    ops, res, no_register = {}, {}, set()
    for f in files:
        text, cur = open(f).read(), None
        for line in text.splitlines():
            m = re.match(r"^([A-Za-z_][\w$.]*):", line)
            if m and re.search(r"^\s*\.type\s+%s,@function" % re.escape(m.group(1)), text, re.M):
                cur = ops.setdefault(m.group(1), collections.Counter())
            elif line.startswith("\t.section"):
                cur = None
            elif cur is not None and (m := re.match(r"^\s+([a-z][a-z0-9_]+)(?:\s+([^;]*))?", line)):
                cur[m.group(1)] += 1
                if not REGISTER.search(m.group(2) or ""):
                    no_register.add(m.group(1))
        # one block per entry of the metadata's kernel list (its items are the two-space-indented "- "; arguments sit deeper)
        for md in re.split(r"\n  - ", text[text.find("amdhsa.kernels:"):] if "amdhsa.kernels:" in text else ""):
            name = re.search(r"\n    \.name:\s*(\S+)", "\n    " + md)        # the entry's own key, not an argument's
            if name and name.group(1) in ops:                               # (a key the compiler did not write is an error)
                res[name.group(1)] = {k: int(re.search(r"(?:^|\n    )" + re.escape(key) + r":\s*(\d+)", md).group(1))
                                      for k, key in RESOURCES}
    return {k: (res[k], ops[k]) for k in res}, no_register


def main(old, new, renames=(), common=False):
    (a, na), (b, nb) = kernels(old), kernels(new)
    for pattern, repl in renames:
        renamed = {re.sub(pattern, repl, name): v for name, v in b.items()}
        if len(renamed) != len(b):
            sys.exit(f"--rename {pattern}={repl}: two kernels of NEW get the same name")
        b = renamed
    no_register = na | nb
    bad = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"{name}\n  MISSING in {'old' if name not in a else 'new'}" + ("  (not compared: --common)" if common else ""))
            bad += not common
            continue
        (ra, oa), (rb, ob) = a[name], b[name]
        diff = {o: (oa[o], ob[o]) for o in set(oa) | set(ob) if oa[o] != ob[o]}
        hard = sorted(o for o in diff if o != PADDING and (not o.startswith("s_") or "dword" in o or o in no_register))
        verdict = "FAIL" if ra != rb or hard else ("same but scalar ALU" if diff else "same")
        bad += verdict == "FAIL"
        print(f"{name}\n  " + "  ".join(f"{k} {ra[k]}" + ("" if ra[k] == rb[k] else f" -> {rb[k]} !") for k, _ in RESOURCES) +
              f"  instructions {sum(oa.values())} -> {sum(ob.values())}  [{verdict}]")
        for o in sorted(diff):
            print(f"    {o:28s} {diff[o][0]:6d} -> {diff[o][1]:6d}" + ("   <-- not scalar ALU" if o in hard else "   (padding)" if o == PADDING else ""))
    print(f"{len(set(a) | set(b))} kernels, {bad} outside the gate")
    return 1 if bad else 0


if __name__ == "__main__":
    args, renames = sys.argv[1:], []
    while "--rename" in args:
        i = args.index("--rename")
        if i + 1 >= len(args) or "=" not in args[i + 1]:
            sys.exit(__doc__)
        renames.append(tuple(args[i + 1].split("=", 1)))
        del args[i:i + 2]
    common = "--common" in args
    args = [x for x in args if x != "--common"]
    if len(args) != 2:
        sys.exit(__doc__)
    sys.exit(main(args[0], args[1], renames, common))
