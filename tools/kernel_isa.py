"""Instruction mix of one kernel of the built library (gfx950 code object).  usage: python tools/kernel_isa.py <mangled-name-substring> [top N] [--dump]"""
import os
import re
import sys
from collections import Counter

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import code_object  # noqa: E402

lib = os.path.join(ROOT, "lfinterpolator_amd", "lib", "liblfi_hip.so")
name = sys.argv[1]
symbol, body = next((k, v) for k, v in code_object.bodies(lib).items() if name in k)   # the first in the code object's order
sec = symbol[symbol.index(name):] + ">:\n" + body
if "--dump" in sys.argv:
    print("\n".join(l.split('//')[0].rstrip() for l in sec.splitlines()))
    sys.exit(0)
c = Counter()
for line in sec.splitlines():
    m = re.match(r'\s+(\w+)', line)
    if m:
        c[m.group(1)] += 1
print(c.most_common(int(sys.argv[2]) if len(sys.argv) > 2 else 14))
