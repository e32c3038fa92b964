"""GPU (-m gpu): every input writer against every reader of a derived input copy — the table of tests/input_writers.py on one context whose
copies were BUILT BEFORE the write.

Per writer and shape, one context: inputs A and the parameters; every reader once (this builds the planar copy, the focus estimate's padded
planes and the per-view pad slots, and checks them); the writer; every reader again, the first of them with no host wait between the writer
and its launch — the view layout, the per-view rows and the poison of what it writes are set up before the writer — and in an order that
rotates from writer to writer; every reader a third time (reuse after the refresh).  Every read is held to the CPU oracle on the shadow grid
the host carries along: `==`, and TEN_WM within one LSB of M16 and inside the interval of the exact sum, as fuzz_cases.fuzz_blend holds it.

Only what a read writes is poisoned before it (LFI_POISON_VIEWS, LFI_POISON_MAPS, LFI_POISON_VIEW_MAPS).  LFI_POISON_DERIVED and
LFI_POISON_FOCUS_WORKSPACE are never used here: they reset grid_version and pad_version and would hide exactly the stale copy under test.

test_long_lived_context_sequence walks one context through 40 steps of writers, state changers (parameters that grow and shrink the copies'
padding, another block radius, the focus steps, the view layout, the input siting, lfi_prepare's eager refresh) and readers in a fixed
shuffled order, the last six after lfi_release_inputs, the shadow grid and the shadow parameters carried along.

Limits: at these shapes a missing stream wait may go unobserved — the copies take microseconds.  These tests hold the version bookkeeping
and the routing; they do not hold the races.  test_gpu_plumbing.py::test_stream_switch_orders_derived_state and the "no host wait in between"
tests of the upload files remain the ordering tests."""
import numpy as np
import pytest

import lfinterpolator_amd as L
import input_writers as iw

pytestmark = pytest.mark.gpu


def _context(gpu, oc, shape, released=False):
    s = iw.Shadow(shape, iw.first_grid(oc, shape))
    ctx = gpu.Context(0)
    ctx.set_grid(shape.cols, shape.rows, shape.W, shape.H)
    ctx.upload_grid(s.grid)
    ctx.set_params(s.params(L))
    if released:
        ctx.render("TEN_WM")      # one render, then the planar copy becomes the only copy
        ctx.release_inputs()
        s.released = True
    return ctx, s


def _read(ctx, s, reader, oc, what, prepared=False, fixed=True):
    if not prepared:
        reader.prepare(L, ctx, s, fixed)
    got = reader.read(L, ctx, s)
    reader.done(ctx)
    try:
        reader.check(got, reader.want(oc, L, s, ctx))
    except AssertionError as e:
        raise AssertionError(f"{what}: {reader.name}: {e}") from None


def _write(ctx, s, writer, oc, seed, keep):
    """apply the writer to the context and to the shadow"""
    env = iw.Env(L, oc, s.shape, seed, s.siting, s.params(L))
    payload = writer.make(env)
    writer.apply(L, ctx, payload, env, keep)
    s.grid = iw.shadow_apply(s.grid, payload, writer)


@pytest.mark.parametrize("shape", iw.SHAPES, ids=lambda s: s.name)
@pytest.mark.parametrize("writer", iw.WRITERS, ids=lambda w: w.name)
def test_writer_reaches_every_reader(writer, shape, gpu, oracle_c):
    keep = []
    ctx, s = _context(gpu, oracle_c, shape, writer.released)
    readers = iw.readers_of(writer)
    done = []
    for r in readers:
        _read(ctx, s, r, oracle_c, "before the writer")
        done.append(r.name)
    turn = (iw.WRITERS.index(writer) + iw.SHAPES.index(shape)) % len(readers)
    order = readers[turn:] + readers[:turn]
    order[0].prepare(L, ctx, s)
    _write(ctx, s, writer, oracle_c, 1, keep)     # … and no ctx.sync() or upload_wait() before the first read
    for i, r in enumerate(order):
        _read(ctx, s, r, oracle_c, f"after {writer.name}, read {i}", prepared=i == 0)
        done.append(r.name)
    for r in readers:
        _read(ctx, s, r, oracle_c, f"after {writer.name}, again")
        done.append(r.name)
    assert sorted(done) == sorted(3 * [r.name for r in readers])   # every pair of this writer ran, three times
    ctx.close()
    del keep


def test_the_pair_count():
    """what the parametrised test above executes: every non-excluded writer with every reader that applies to its context"""
    pairs = iw.pairs()
    rgba = [w for w in iw.WRITERS if not w.released]
    assert len(pairs) == len(rgba) * len(iw.readers_of(False)) + (len(iw.WRITERS) - len(rgba)) * len(iw.readers_of(True))
    print(f"{len(iw.WRITERS)} writers, {len(pairs)} (writer, reader) pairs per shape, {len(iw.SHAPES)} shapes")


# ---- one long-lived context -----------------------------------------------------------------------------------------------------------------------

def _toggle_focus(ctx, s):
    s.focus = iw.FOCUS_LARGE if s.focus == iw.FOCUS else iw.FOCUS     # the larger one grows planar_reach and pad_shift
    ctx.set_params(s.params(L))


def _toggle_radius(ctx, s):
    s.radius = s.shape.radius2 if s.radius is None else None
    ctx.set_params(s.params(L))


def _toggle_steps(ctx, s):
    s.steps = 64 if s.steps == 32 else 32
    ctx.set_focus_steps(s.steps)


def _toggle_layout(ctx, s):
    s.layout = "planar" if s.layout == "rgba" else "rgba"
    ctx.set_output_layout(s.layout)


def _toggle_siting(ctx, s):
    s.siting = "left" if s.siting == "centre" else "centre"
    ctx.set_yuv_siting(s.siting, "centre")


def _prepare(ctx, s):
    ctx.prepare("TEN_WM")    # turns on eager_planar: images that arrive from now on refresh their planes at once


CHANGERS = {"focus": _toggle_focus, "block_radius": _toggle_radius, "focus_steps": _toggle_steps, "output_layout": _toggle_layout,
            "yuv_siting": _toggle_siting, "prepare_ten_wm": _prepare}


def _schedule():
    rng = np.random.default_rng(20261)
    writers = [w for w in iw.WRITERS if not w.released]
    flagged = iw.FLAGGED_READERS
    readers = [r for r in iw.readers_of(False) if r not in flagged]
    lean_readers = [r for r in iw.readers_of(True) if r not in flagged]
    steps = [("change", c) for c in CHANGERS if c != "prepare_ten_wm"] * 2 + [("change", "prepare_ten_wm")]
    steps += [("write", writers[i]) for i in rng.choice(len(writers), 11, replace=False)]
    # every unflagged reader once; the two drawn reads are flagged ones — all four of which are also read before the release and at the end
    steps += [("read", r) for r in readers] + [("read", flagged[i]) for i in rng.choice(len(flagged), 12 - len(readers), replace=False)]
    steps = [steps[i] for i in rng.permutation(len(steps))]
    lean = [w for w in iw.WRITERS if w.released]
    steps += [step for i, w in enumerate(lean) for step in (("write", w), ("read", lean_readers[i % len(lean_readers)]))]
    assert len(steps) == 40 and len(lean) == 3 and len(flagged) == 4
    return steps


def test_long_lived_context_sequence(gpu, oracle_c):
    """40 steps on one context, fixed seed.  34 shuffled steps while the context holds its RGBA inputs: 11 writers, every state changer (each
    toggle twice: there and back; lfi_prepare once) and 12 reads (every unflagged reader once, and two drawn flagged ones).  Then every
    reader the state admits, the four flagged ones among them, lfi_release_inputs, and 6 steps on the released context: each of its writers
    followed by a read; at the end every reader of a released context, the flagged ones again.  The fixed-focus readers render in the view
    layout the steps left (the flagged ones set the planar layout, which their flags need); the plain estimate, which computes 32 candidates
    only, gives way to the factored one while lfi_set_focus_steps is 64.  What the flagged readers cost the earlier ones, the 40 steps kept:
    the two drawn reads used to be second reads of unflagged readers; and a flagged read leaves the view layout planar until the next
    output_layout step, so the Std and Ten reads behind it render planar more often than a schedule without flagged reads would have them."""
    shape = iw.SHAPES[0]
    readers, lean_readers = iw.readers_of(False), iw.readers_of(True)
    steps = _schedule()
    keep, log = [], []
    ctx, s = _context(gpu, oracle_c, shape)
    try:
        for i, (kind, what) in enumerate(steps):
            if kind == "write" and what.released and not s.released:
                for r in readers:     # every reader that the state admits, then the release
                    if not (s.steps != 32 and r.variant == "plain"):
                        log.append(f"before the release: read {r.name}")
                        _read(ctx, s, r, oracle_c, "before the release", fixed=False)
                log.append("release_inputs")
                ctx.release_inputs()
                s.released = True
            if kind == "change":
                log.append(f"{i}: change {what}")
                CHANGERS[what](ctx, s)
            elif kind == "write":
                log.append(f"{i}: write {what.name} {what.image_runs(shape.n)}")
                _write(ctx, s, what, oracle_c, 100 + i, keep)
            else:
                if s.steps != 32 and what.variant == "plain":
                    what = next(r for r in readers if r.variant == "factored")
                log.append(f"{i}: read {what.name} (focus {s.focus}, radius {s.radius}, steps {s.steps}, {s.layout}, {s.siting})")
                _read(ctx, s, what, oracle_c, f"step {i}", fixed=False)
        for r in lean_readers:
            log.append(f"end: read {r.name}")
            _read(ctx, s, r, oracle_c, "at the end", fixed=False)
    except Exception:
        print("\n".join(log))
        raise
    ctx.close()
    del keep
