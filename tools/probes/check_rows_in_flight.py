#!/usr/bin/env python3
"""check_inflight.py file.s [kernel-name-substring]: the SGPRs an inline-asm s_load of the
rows-ahead core writes are not touched until the next `s_waitcnt lgkmcnt(0)`."""
import re
import sys

src = open(sys.argv[1]).read().split("\n")
want = sys.argv[2] if len(sys.argv) > 2 else ""
REG = re.compile(r"\bs\[(\d+):(\d+)\]|\bs(\d+)\b")


def regs(text):
    out = set()
    for m in REG.finditer(text):
        if m.group(1):
            out |= set(range(int(m.group(1)), int(m.group(2)) + 1))
        else:
            out.add(int(m.group(3)))
    return out


kernel, in_asm, flight, bad, blocks = None, False, set(), 0, 0
for ln, l in enumerate(src, 1):
    t = l.strip()
    if re.match(r"^[_A-Za-z]\w*:", l):
        kernel, flight = t.split(":")[0], set()
        continue
    if kernel is None or want not in kernel:
        continue
    if t.startswith(";;#ASMSTART"):
        in_asm = True
        continue
    if t.startswith(";;#ASMEND"):
        in_asm = False
        continue
    if not t or t.startswith((";", ".")):
        continue
    code = t.split(";")[0]
    if in_asm and code.startswith("s_waitcnt") and "lgkmcnt(0)" in code:
        flight = set()
        continue
    if in_asm and code.startswith("s_load_dword"):
        ops = code.split(None, 1)[1].split(",")
        if regs(",".join(ops[1:])) & flight:
            print("address in flight", kernel[:40], ln, t); bad += 1
        flight |= regs(ops[0])
        blocks += 1
        continue
    if flight and regs(code) & flight:
        print("touches in-flight SGPRs", kernel[:60], ln, t)
        bad += 1
    if flight and code.startswith(("s_cbranch", "s_branch", "s_endpgm", "s_barrier")):
        print("control flow with rows in flight", kernel[:60], ln, t)
        bad += 1
print("asm s_loads:", blocks, "violations:", bad)
sys.exit(1 if bad else 0)
