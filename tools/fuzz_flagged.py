"""Soak run of tests/fuzz_cases.py::fuzz_flagged (the pytest suite runs 24 + 2 cases per flag with fixed seeds: tests/test_gpu_fuzz.py).
usage: python tools/fuzz_flagged.py [deep|in_frame|linear|all] [cases] [seed]"""
import os
import sys
sys.path.insert(0, ".")
sys.path.insert(0, os.path.join(".", "tests"))
import fuzz_cases
import lfinterpolator_amd as L
from oracle import lfi_oracle_c as oc

FLAGS = {"deep": L.LFI_FLAG_DEEP_VIEWS, "in_frame": L.LFI_FLAG_IN_FRAME, "linear": L.LFI_FLAG_LINEAR_LIGHT}
which = sys.argv[1] if len(sys.argv) > 1 else "all"
n_cases = int(sys.argv[2]) if len(sys.argv) > 2 else 96
seed = int(sys.argv[3]) if len(sys.argv) > 3 else 5
total = 0
for name in (FLAGS if which == "all" else [which]):
    bad = fuzz_cases.fuzz_flagged(L, oc, FLAGS[name], n_cases, seed, log=lambda s: print(name, s, flush=True))
    for b in bad:
        print("MISMATCH", name, b)
    print("done:", name, n_cases, "+ 2 cases,", len(bad), "mismatches")
    total += len(bad)
sys.exit(1 if total else 0)
