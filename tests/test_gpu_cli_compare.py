"""GPU (-m gpu): the command line's --compare DIR and --compare-methods (the reference's scripts/compareDirs.sh on the device).

The printed lines are parsed and held against tests/quality_ref.py on the PNG files read back.  The values are printed with nine significant
digits, which rounds them by up to 5e-9 of their size: printed values are compared to rtol 1e-8; the integers exactly."""
import math
import re

import numpy as np
import pytest
from PIL import Image

import quality_ref as ref
from view_rows import run_cli

pytestmark = pytest.mark.gpu

VIEWS = 6
W, H = 150, 61
BASE = ["--synthetic", f"4,4,{W},{H}", "-t", "0,0.5,1,0.5", "-f", "0.1", "-n", str(VIEWS), "-b", "1"]
# The API's tolerances (ssim rtol 1e-9, psnr 1e-9 dB: tests/test_gpu_compare_views.py) cannot be read off text of nine significant digits
# (setprecision(9), the format the CLI prints all its results in): a printed value is within 5e-9 of its size, hence 1e-8 for PRINTED values only.
PRINTED_RTOL = 1e-8
LINE = re.compile(r"^compare (\d\d) psnr (\S+) ssim (\S+) maxdiff (\d+) differing (\d+)$", re.M)
ALL = re.compile(r"^compare all psnr (\S+) ssim (\S+)$", re.M)


def _parse(stdout):
    views = [(int(m.group(1)), float(m.group(2)), float(m.group(3)), int(m.group(4)), int(m.group(5))) for m in LINE.finditer(stdout)]
    total = ALL.findall(stdout)
    assert len(total) == 1, stdout
    return views, (float(total[0][0]), float(total[0][1]))


def _close(x, y, rtol):
    return x == y if math.isinf(x) or math.isinf(y) else abs(x - y) <= rtol * abs(y)


def _read(folder):
    return [np.array(Image.open(folder / f"{v:02d}.png")) for v in range(VIEWS)]


def test_cli_compare_with_a_directory_and_with_the_other_method(gpu, tmp_path):
    a, b, c = tmp_path / "A", tmp_path / "B", tmp_path / "C"
    res = run_cli(gpu, *BASE, "-m", "STD", "-o", str(a))
    assert res.returncode == 0, res.stderr
    assert "compare " not in res.stdout
    res = run_cli(gpu, *BASE, "-m", "TEN_WM", "-o", str(b), "--compare", str(a))
    assert res.returncode == 0, res.stderr
    views, total = _parse(res.stdout)
    std, ten = _read(a), _read(b)
    want = [ref.compare(ten[v], std[v]) for v in range(VIEWS)]
    assert [v[0] for v in views] == list(range(VIEWS))
    for (v, psnr, ssim, maxdiff, differing), w in zip(views, want):
        assert (maxdiff, differing) == (w["max_abs_diff"], w["differing_bytes"]), (v, maxdiff, differing, w)
        assert _close(psnr, w["psnr_all"], PRINTED_RTOL) and _close(ssim, w["ssim_all"], PRINTED_RTOL), (v, psnr, ssim, w)
    agg = ref.aggregate(want, W, H)
    assert _close(total[0], agg["psnr_all"], PRINTED_RTOL) and _close(total[1], agg["ssim_all"], PRINTED_RTOL), (total, agg)
    assert any(w["differing_bytes"] for w in want) and max(w["max_abs_diff"] for w in want) <= 1      # two methods, one LSB apart at most

    # --compare-methods: the STD views never leave the device; the same integers, ssim to rtol 1e-9 and psnr to 1e-9 dB of the run above;
    # the stored images are TEN_WM's
    res = run_cli(gpu, *BASE, "-m", "TEN_WM", "-o", str(c), "--compare-methods")
    assert res.returncode == 0, res.stderr
    views2, total2 = _parse(res.stdout)
    assert len(views2) == VIEWS
    for one, two in zip(views, views2):
        assert (one[0], one[3], one[4]) == (two[0], two[3], two[4]), (one, two)
        assert (one[1] == two[1] or abs(one[1] - two[1]) <= 1e-9) and _close(two[2], one[2], 1e-9), (one, two)
    assert (total[0] == total2[0] or abs(total[0] - total2[0]) <= 1e-9) and _close(total2[1], total[1], 1e-9)
    for x, y in zip(_read(c), ten):
        assert (x == y).all()
    # … and the other way round: -m STD compared with TEN_WM gives the same differences (PSNR and the integers are symmetric)
    res = run_cli(gpu, *BASE, "-m", "STD", "-o", str(c), "--compare-methods")
    assert res.returncode == 0, res.stderr
    views3, _ = _parse(res.stdout)
    assert [(v[0], v[3], v[4]) for v in views3] == [(v[0], v[3], v[4]) for v in views]
    for x, y in zip(_read(c), std):
        assert (x == y).all()

    # a view against itself
    res = run_cli(gpu, *BASE, "-m", "STD", "-o", str(c), "--compare", str(a))
    assert res.returncode == 0, res.stderr
    views4, total4 = _parse(res.stdout)
    assert all(v[1] == math.inf and v[3] == 0 and v[4] == 0 for v in views4) and total4[0] == math.inf


def test_cli_compare_refusals(gpu, tmp_path):
    a = tmp_path / "A"
    res = run_cli(gpu, *BASE, "-m", "STD", "-o", str(a))
    assert res.returncode == 0, res.stderr
    # a missing reference file
    (a / "03.png").unlink()
    res = run_cli(gpu, *BASE, "-m", "TEN_WM", "-o", str(tmp_path / "B"), "--compare", str(a))
    assert res.returncode != 0 and "03.png" in res.stderr and "compare 00" not in res.stdout
    # a reference of another size
    Image.fromarray(np.zeros((H, W + 1, 4), np.uint8)).save(a / "03.png")
    res = run_cli(gpu, *BASE, "-m", "TEN_WM", "-o", str(tmp_path / "B"), "--compare", str(a))
    assert res.returncode != 0 and "03.png" in res.stderr and f"{W + 1}x{H}" in res.stderr
    # no directory, both options, more than one GPU
    assert run_cli(gpu, *BASE, "-m", "TEN_WM", "-o", str(tmp_path / "B"), "--compare").returncode != 0
    assert run_cli(gpu, *BASE, "-m", "TEN_WM", "-o", str(tmp_path / "B"), "--compare", str(a), "--compare-methods").returncode != 0
    res = run_cli(gpu, *BASE, "-m", "TEN_WM", "-o", str(tmp_path / "B"), "--compare-methods", "-g", "2")
    assert res.returncode != 0 and "one GPU" in res.stderr
