"""CPU: the interval check of tests/ten_interval.py itself, before the GPU tests lean on it.

quantise() is pinned to the oracle's TEN_EXACT model; the interval stays narrow enough to be a check (a condition the reference alone must
meet on every TEN_WM row of the dispatch table); and it reports the defects that "within one LSB of M16" lets through on 12×12 and 15×15
grids: an input image left out, an image sampled one pixel off, one pixel column of one view wrong.
"""
import numpy as np
import pytest

import poison
import ten_interval as ti
import test_gpu_dispatch_coverage as dc

TRAJ = "0.071,0.071,0.93,0.93"
W, H, V = 200, 4, 8
# (cols, rows, effect): one to four chunks of images, and the small weights of effect 7
SHAPES = [(3, 3, 3.0), (8, 8, 3.0), (9, 9, 3.0), (12, 12, 3.0), (15, 15, 3.0), (15, 15, 7.0)]
MUTATION_SHAPES = SHAPES[3:]
TWO_VALUED_CAP = 0.02


def _id(s):
    return f"{s[0]}x{s[1]}_effect{s[2]:g}"


class _Case:
    def __init__(self, L, oc, shape, smooth=False):
        self.oc = oc
        cols, rows, effect = shape
        n = cols * rows
        self.hp = L.build_params(cols, rows, W, H, TRAJ, 0.23, 0.0, effect, 1.783, V)
        if smooth:   # ramps of a quarter level per pixel from image-dependent levels: neighbouring output columns differ by at most one
            g, y, x, ch = np.ogrid[:n, :H, :W, :4]
            self.lf = ((37 * g + 11 * ch + 3 * y) % 64 + 64 + (x + g % 4) // 4).astype(np.uint8)
            self.lf[..., 3] = 255
        else:
            self.lf = oc.synthetic_lf(n, W, H, 0x5EED + n + W)
        self.S, self.eps = ti.exact_sums(oc, self.lf, self.hp, threads=dc.THREADS)
        self.lo, self.hi = ti.interval(self.S, self.eps)
        self.exact = self.ten(oc.TEN_EXACT)
        self.m16 = self.ten(oc.TEN_M16)

    def ten(self, model):
        return self.oc.blend_ten(self.lf, self.hp.focused_offsets, self.hp.offsets, self.hp.weights, model=model, threads=dc.THREADS)

    def rendered(self, S):
        """The bytes of a kernel that accumulates without error: q of its sums, alpha 255."""
        return np.concatenate([ti.quantise(S), np.full(S.shape[:-1] + (1,), 255, np.uint8)], axis=-1)


@pytest.fixture(scope="module")
def cases(native, oracle_c):
    made = {}

    def get(shape, smooth=False):
        if (shape, smooth) not in made:
            made[shape, smooth] = _Case(native, oracle_c, shape, smooth)
        return made[shape, smooth]
    return get


def test_quantise_ties_saturation_and_sign():
    half = np.float64(2.0 ** -4)                           # half the fp16 spacing in [128, 256)
    # ties: N − 1/16 lies between N − 1/8 (odd mantissa) and N (even) and goes UP to the integer; N + 1/16 and N − 3/16 do not reach one
    s = np.array([0.0, 0.999, 1.0, 199.93, 200.0 - half, 200.0 + half, 200.0 - 3 * half, 254.93, 255.0 - half, 300.0, 1e6, -0.5, -3.0, 2.0 ** -30])
    assert ti.quantise(s).tolist() == [0, 0, 1, 199, 200, 200, 199, 254, 255, 255, 255, 0, 0, 0]
    assert ti.quantise(np.array([200.0 - half - 2.0 ** -30, 100.0 - half / 2, 100.0 - half / 2 - 2.0 ** -30])).tolist() == [199, 100, 99]
    assert ti.ties(s) == 4 and ti.ties(np.array([200.0 - half, 3.0, 0.25 + 2.0 ** -13, 256.0 + half])) == 2


def test_epsilon_is_the_analytic_std_bound_per_addend():
    one, tiny = np.float16(1.0).view(np.uint16), np.float16(2.0 ** -20).view(np.uint16)
    w = np.zeros((4, 9), np.uint16)
    w[0, :2] = one                                         # Σw = 2: B = 510 < 512
    w[1, :3] = one                                         # Σw = 3: B = 765: partial sums reach [512, 1024)
    w[2, :] = tiny
    w[3, 0] = np.float16(-2.5).view(np.uint16)             # |w|: B = 637.5
    assert ti.epsilon(w, 9).tolist() == [16 * 2.0 ** -15, 16 * 2.0 ** -14, 16 * 2.0 ** -15, 16 * 2.0 ** -14]
    assert ti.epsilon(w[:1, :], 225).tolist() == [240 * 2.0 ** -15] and ti.epsilon(w[:1], 64).tolist() == [64 * 2.0 ** -15]


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_quantise_is_the_oracles_exact_model_and_lies_inside(shape, cases):
    c = cases(shape)
    assert (c.rendered(c.S) == c.exact).all()
    assert ti.outside(c.exact, c.lo, c.hi) == 0
    width = c.hi.astype(int) - c.lo.astype(int)
    print(f"TEN_INTERVAL_CPU {_id(shape)} k_pad={(shape[0] * shape[1] + 15) // 16 * 16} two_valued={(width == 1).mean():.4%} widest={width.max()} "
          f"m16_outside={((c.m16[..., :3] < c.lo) | (c.m16[..., :3] > c.hi)).mean():.2%}")
    assert width.min() >= 0 and width.max() <= 1 and (width == 1).mean() <= TWO_VALUED_CAP
    assert poison.mismatch(c.m16, c.exact, 1) == 0


def test_report_gives_the_error_a_byte_needed(cases):
    c = cases(SHAPES[1])
    assert ti.report(c.exact, c.S, c.eps).size == 0
    got = c.exact.copy()
    v, y, x, ch = 3, 2, 77, 1
    s = c.S[v, y, x, ch]
    got[v, y, x, ch] = ti.quantise(s) + 2
    need = ti.report(got, c.S, c.eps)
    assert ti.outside(got, c.lo, c.hi) == 1 and need.shape == (1,)
    d = need[0] * c.eps[v]
    assert 1.0 - 0.0625 <= d <= 2.0 + 0.0625                # two integers up, less where s stood in its own, within one fp16 rounding
    assert ti.quantise(s + d) == got[v, y, x, ch] and ti.quantise(s + d * (1 - 1e-9)) < got[v, y, x, ch]
    got[v, y, x, ch] = ti.quantise(s) - 1
    d = ti.report(got, c.S, c.eps)[0] * c.eps[v]
    assert ti.quantise(s - d) == got[v, y, x, ch] and ti.quantise(s - d * (1 - 1e-9)) > got[v, y, x, ch]
    got[0, 0, 0, 3] = 254
    with pytest.raises(AssertionError):
        ti.outside(got, c.lo, c.hi)


TEN_ROWS = [r for r in dc.MATRIX if r.method == "TEN_WM" and not r.flags & dc.ROUND]


@pytest.mark.parametrize("row", TEN_ROWS, ids=lambda r: r.name)
def test_interval_stays_a_check_on_every_dispatch_row(row, native, oracle_c):
    """A condition on the reference alone, not a measurement of a kernel: on the row's own inputs at most 2 % of the bytes have two admissible
    values, none has three, and the exact model lies inside.  (Rows that walk a tile loop: 16 image rows here.)  The dyadic rows' preconditions
    (multiples of 2^-12, sums ≤ 2, enough fp16 ties) are asserted by ten_row_interval, as before their launch."""
    hp, lf, m = dc.row_inputs(native, oracle_c, row, 16 if row.persistent else row.H)
    S, eps, lo, hi = (a[row.v0:row.v1] for a in dc.ten_row_interval(oracle_c, row, hp, lf, m))
    width = hi.astype(int) - lo.astype(int)
    assert width.min() >= 0 and width.max() <= 1, (row.name, width.min(), width.max())
    assert (width == 1).mean() <= TWO_VALUED_CAP, (row.name, (width == 1).mean())
    q = ti.quantise(S)
    assert ((lo <= q) & (q <= hi)).all()
    if row.weights == "dyadic":
        assert (eps == 0).all() and (lo == hi).all()
    elif row.weights == "default":
        assert (eps == (row.n + 15) // 16 * 16 * 2.0 ** -15).all()
    else:
        assert (eps > (row.n + 15) // 16 * 16 * 2.0 ** -15).all()


def _old_check_passes(got, m16):
    return poison.mismatch(got, m16, 1) == 0


@pytest.mark.parametrize("shape", MUTATION_SHAPES, ids=_id)
def test_interval_reports_a_dropped_image(shape, cases, oracle_c):
    """The image with the smallest non-zero mean weight contributes nothing: within one LSB of M16 everywhere, outside the interval in
    more than 1 % of the bytes."""
    c = cases(shape)
    w = ti.weights_f64(c.hp.weights)
    mean = np.where(w.mean(axis=0) > 0, w.mean(axis=0), np.inf)
    g = int(mean.argmin())
    assert np.isfinite(mean[g])
    keep = c.hp.weights
    c.hp.weights = keep.copy()
    c.hp.weights[:, g] = 0
    try:
        mut = c.rendered(ti.exact_sums(oracle_c, c.lf, c.hp, threads=dc.THREADS)[0])
    finally:
        c.hp.weights = keep
    share = ti.outside(mut, c.lo, c.hi) / c.lo.size
    print(f"TEN_INTERVAL_CPU {_id(shape)} dropped image {g} (mean weight {mean[g]:.2g}): max diff from M16 "
          f"{np.abs(mut.astype(int) - c.m16.astype(int)).max()}, outside {share:.2%}")
    assert _old_check_passes(mut, c.m16)
    assert share > 0.01


@pytest.mark.parametrize("shape", MUTATION_SHAPES[:2], ids=_id)
def test_interval_reports_an_image_sampled_one_pixel_off(shape, cases, oracle_c):
    """The image with the largest offset (of those equally far out, the one of least weight) is read one pixel to the right.  (Effect 3 only:
    at effect 7 that image's mean weight is 2e-4 and the mutant leaves the interval in 0.98 % of the bytes, below the 1 % asked for here.)"""
    c = cases(shape)
    w = ti.weights_f64(c.hp.weights).mean(axis=0)
    far = np.abs(c.hp.focused_offsets.astype(np.int64)).sum(axis=1)
    g = min((i for i in range(len(far)) if far[i] == far.max()), key=lambda i: w[i])
    keep = c.hp.focused_offsets
    c.hp.focused_offsets = keep.copy()
    c.hp.focused_offsets[g, 0] += 1
    try:
        mut = c.rendered(ti.exact_sums(oracle_c, c.lf, c.hp, threads=dc.THREADS)[0])
    finally:
        c.hp.focused_offsets = keep
    share = ti.outside(mut, c.lo, c.hi) / c.lo.size
    print(f"TEN_INTERVAL_CPU {_id(shape)} image {g} (offset {keep[g].tolist()}, mean weight {w[g]:.2g}) one pixel off: max diff from M16 "
          f"{np.abs(mut.astype(int) - c.m16.astype(int)).max()}, outside {share:.2%}")
    assert _old_check_passes(mut, c.m16)
    assert share > 0.01


@pytest.mark.parametrize("shape", MUTATION_SHAPES, ids=_id)
def test_interval_reports_one_wrong_pixel_column(shape, cases):
    """One pixel column of one view holds its neighbour's bytes: fewer than 0.1 % of the bytes differ from the exact model and none is
    further than one LSB from M16, so both older checks pass; the interval does not.  (Inputs smooth along x, so that a neighbouring column
    can be that close at all; the synthetic images differ by 8 levels from one column to the next.)"""
    c = cases(shape, smooth=True)
    assert ti.outside(c.exact, c.lo, c.hi) == 0 and (c.rendered(c.S) == c.exact).all()
    for v, x in ((v, x) for v in range(V) for x in range(W - 1)):
        mut = c.exact.copy()
        mut[v, :, x] = mut[v, :, x + 1]
        if _old_check_passes(mut, c.m16) and ti.outside(mut, c.lo, c.hi) > 0:
            break
    else:
        pytest.fail("no column whose neighbour is within one LSB of M16 and differs from it")
    assert (mut != c.exact).mean() < 1e-3                   # the fraction check of the golden-fixture tests would have let it through
    assert _old_check_passes(mut, c.m16)
    assert ti.outside(mut, c.lo, c.hi) > 0
