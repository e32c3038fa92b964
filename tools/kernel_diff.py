"""Which kernels of two builds of the library differ in their instructions (gfx950 code objects; addresses, encodings and the section's
trailing padding left out).  usage: python tools/kernel_diff.py <liblfi_hip.so> <liblfi_hip.so>"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
import code_object  # noqa: E402


def instructions(lib):
    # "\tv_mov_b32 v0, v1    // 000000001234: 7E000301" -> "v_mov_b32 v0, v1"; "..." is the padding behind the section's last symbol
    return {k: [l.split("//")[0].strip() for l in v.splitlines() if l.strip() not in ("", "...")] for k, v in code_object.bodies(lib).items()}


a, b = instructions(sys.argv[1]), instructions(sys.argv[2])
differing = sorted(k for k in set(a) | set(b) if a.get(k) != b.get(k))
print(f"{len(a)} and {len(b)} symbols ({len(code_object.kernels(sys.argv[1]))} and {len(code_object.kernels(sys.argv[2]))} kernels), "
      f"{sum(map(len, a.values()))} and {sum(map(len, b.values()))} instructions, {len(differing)} symbols differ")
for k in differing:
    print(("only in the first: " if k not in b else "only in the second: " if k not in a else "differs: ") + k)
sys.exit(1 if differing else 0)
