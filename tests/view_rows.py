"""Helpers shared by the per-view-rows GPU tests (test_gpu_view_focus.py, test_gpu_view_centres.py): the per-view check against the
oracle and the CLI runner."""
import subprocess

import numpy as np

TEN_TOL_LSB = 1


def check_views(got, want, method):
    """got: the rendered views; want: per view the oracle's STD view, or for TEN_WM its (M16, exact) pair.  STD byte for byte, TEN_WM
    within the TEN_WM contract (≤ TEN_TOL_LSB from M16, < 1e-3 of the bytes off the exactly-summed model)."""
    if method == "STD":
        for v, w in enumerate(want):
            assert (got[v] == w).all(), ("STD view", v, int((got[v] != w).sum()))
    else:
        m16 = np.stack([w[0] for w in want])
        exact = np.stack([w[1] for w in want])
        assert np.abs(got.astype(int) - m16.astype(int)).max() <= TEN_TOL_LSB
        assert (got != exact).mean() < 1e-3
        assert (got[..., 3] == 255).all()


def run_cli(native, *args):
    return subprocess.run([native.build.CLI, *args], capture_output=True, text=True, timeout=300)
