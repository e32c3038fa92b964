"""Register / LDS / scratch use of every kernel in the built library (from the gfx950 code object's metadata).
usage: python tools/kernel_regs.py [substring]"""
import os
import subprocess
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, os.path.join(ROOT, "tests"))
import code_object  # noqa: E402

lib = os.path.join(ROOT, "lfinterpolator_amd", "lib", "liblfi_hip.so")
filt = sys.argv[1] if len(sys.argv) > 1 else ""
for name, r in code_object.kernels(lib).items():
    if filt in name:
        demangled = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        print(f"{demangled[:90]:90s} vgpr {r['.vgpr_count']:3d} agpr {r['.agpr_count']:3d} sgpr {r['.sgpr_count']:3d} "
              f"spill {r['.vgpr_spill_count']} scratch {r['.private_segment_fixed_size']} lds {r['.group_segment_fixed_size']}")
