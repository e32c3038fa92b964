"""Every call that changes what a context answers (CHANGES) against every call that reads a context's state (PROBES): is a context that was
used in one state and then taken to another the same as a fresh context brought straight there?

A context carries about forty device buffers and as many cached host values (planar_pitch / planar_padx / planar_reach, planar_phase,
pad_version / pad_shift / pad_ids, launches_with_offsets, view_offsets_reach, param_total and the two parameter halves, deep_v0 / deep_v1,
kept_v0 / kept_n, eager_planar, weights_scalable …).  Whether each is right after a state-changing call rests on the hand-placed release groups
of csrc/hip/lfi_context.hpp (free_params, free_view_rows, free_views, drop_kept, drop_inputs, drop_stage_plane, free_grid, touch_all,
drop_deep_range) and on the "grow" / "exact" policy of each buffer in the Lifetimes table of DESIGN.md §3.  A buffer kept too long renders a
plausible picture of the previous state, so nothing but a comparison with the right answer shows it.

This file is the table both tests walk: tests/test_context_reuse_table.py (CPU: every function of include/lfi.h is classified, every size
grows and shrinks alone somewhere, and no change whose outputs keep their shape could pass on the previous state's answer) and
tests/test_gpu_context_reuse.py (GPU: every change on a context that was worked in the before-state, beside a fresh context; one long-lived
context through a seeded walk).  It imports without a GPU.

A State is everything that fixes what a context answers; `move` issues the calls that take a context from one state to the next — only the
calls a caller must make: what a change invalidates (uploads after new input planes, lfi_set_params after a new grid or window, per-view rows
after new parameters) is repeated, nothing else is.  A fresh context is `move` from no state at all, so both contexts go through one code path.

A probe reads the context and is held to the CPU oracle or to a restatement under tests/ on the state's shadow (input_writers.Shadow).  In a
state where include/lfi.h refuses the probe's call, the check is the refusal: its message, and lfi_memory_info unchanged.  In a state where a
probe makes no statement its mode is a skip with the reason, by name (SKIP …): nothing is passed silently.

The STD and TEN_WM variants (lfi_set_variant) are a setting of the state: std and ten_wm render by whatever the context holds and assert the
kernel's name where the state names another kernel; the readers taken from input_writers set "auto" for themselves and the state's variants are
put back behind them.  The FOCUS variants belong to the focus-map probes, which run under three.

Limits.  No stream races (tests/stream_order.py holds those).  Under a row
window the held rows are those of the fixed-focus offsets, so the all-focus readers are held to their refusal there;
tests/dispatch_windows.py renders all-focus bands.  A context after lfi_release_inputs changes neither focus nor weights: what the planar
copy alone serves then depends on the padding it was built with (tests/test_gpu_plumbing.py::test_release_inputs).
"""
import ctypes
from dataclasses import dataclass, replace

import numpy as np

import lfinterpolator_amd as L
import deep_ref
import inframe_ref
import input_writers as iw
import linear_ref
import native_filter_ref
import native_ref
import poison
import quality_ref
import quilt_yuv_ref
import rgbd_yuv_ref
import scaled_quilt_ref
import ten_interval
import yuv10_ref
import yuv_left_ref
import yuv_ref
import yuv_surfaces_ref as sref

DEEP, IN_FRAME, PER_BATCH, LINEAR = L.LFI_FLAG_DEEP_VIEWS, L.LFI_FLAG_IN_FRAME, L.LFI_FLAG_TEN_ROUND_PER_BATCH, L.LFI_FLAG_LINEAR_LIGHT
# the parameter flags that send a fixed-focus render to launch_flagged_views (deep_blend, blend_inframe, blend_linear): every predicate on "a
# flagged state" goes through this one mask, so that the next such flag is added here and nowhere else
VIEW_FLAGS = DEEP | IN_FRAME | LINEAR
# what may be poisoned between the work and the change: never LFI_POISON_DERIVED or LFI_POISON_FOCUS_WORKSPACE — they reset grid_version and
# pad_version, the bookkeeping under test (input_writers.Reader)
POISON_BITS = L.LFI_POISON_VIEWS | L.LFI_POISON_SCRATCH | L.LFI_POISON_MAPS | L.LFI_POISON_VIEW_MAPS | L.LFI_POISON_DEEP


def poison_bits(before, after, again=None):
    """POISON_BITS, but for the per-view maps where they are part of the state the change keeps: estimated by lfi_view_focus_maps for rows that
    no call of the change sets again"""
    kept = (before.rows_kind == after.rows_kind == "view_maps" and again is None and before.dims == after.dims and before.window == after.window
            and before.params_key() == after.params_key())
    return POISON_BITS & ~L.LFI_POISON_VIEW_MAPS if kept else POISON_BITS


# ---- states -------------------------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class State:
    cols: int
    rows: int
    W: int
    H: int
    V: int = 5
    window: tuple = None       # None, or the output rows (o0, o1) of lfi_set_row_window; the held input rows are L.input_rows of them.  (0, H): the call, and no window
    inputs: str = "owned"      # "owned" / "attached" (lfi_attach_grid + lfi_grid_modified) / "released" (lfi_release_inputs)
    focus: float = 0.05
    rng: float = iw.RANGE
    radius: tuple = None       # None: build_params'
    ids: int = 9               # the first `ids` focus ids of build_params
    flags: int = 0
    wide: bool = False         # weights outside [0, 2)
    layout: str = "rgba"
    views: int = 0             # 0: the context's own views; else lfi_attach_views of a caller's buffer that holds this many views
    steps: int = 32
    siting: tuple = ("centre", "centre")
    stream: str = "own"        # or "caller"
    variant: tuple = ("auto", "auto")   # lfi_set_variant of STD and TEN_WM: a context setting.  (The FOCUS variants are set by the focus-map probes.)
    rows_kind: str = None      # per-view rows set on the context: None / "int" / "float" / "view_maps"
    seed: int = 0x1F1F

    @property
    def n(self):
        return self.cols * self.rows

    @property
    def dims(self):
        return (self.cols, self.rows, self.W, self.H)

    @property
    def siting_in(self):
        return self.siting[0]

    @property
    def siting_out(self):
        return self.siting[1]

    @property
    def windowed(self):
        return self.window is not None and self.window != (0, self.H)

    @property
    def band(self):
        return self.window if self.windowed else (0, self.H)

    def params_key(self):
        return (self.V, self.focus, self.rng, self.radius, self.ids, self.flags, self.wide)

    def want_key(self):
        """what an expected output depends on"""
        return self.dims + self.params_key() + (self.steps, self.siting, self.rows_kind, self.seed)


# the smallest shapes at which the machinery is live.  136: a multiple of 8 and not of 128, two 128-pixel tiles, the second ragged.  72
# images: two chunks of 64 with k_pad 80; 70 views: a second view pass; 300: no multiple of 8, the planar view pitch is padded.  W and H even.
SMALL = State(3, 3, 136, 24, V=5)
LARGE = State(9, 8, 300, 40, V=70)
TALL = replace(SMALL, H=40)     # room for interior bands: at focus 0.05 the fixed-focus offsets reach one row
AUTO = ("auto", "auto")
OTHER_KERNELS = ("persist_m2_nt", "wave_m2_nt")     # both honour a row window
KERNEL_OF = {"persist_m2_nt": "blend_persist<STD>", "wave_m2_nt": "blend_wave<TEN_WM>"}


def ten_kernel_of(st):
    """the TEN_WM kernel of a state whose variant is not "auto": the wave-private kernels serve one view pass (route_blend: wave_fits needs
    v1 − v0 <= 64 and one chunk of images), so over 64 views the variant gives way to the persistent kernel"""
    return KERNEL_OF[st.variant[1]] if st.V <= 64 and st.n <= 64 else "blend_persist<TEN_WM>"

_grids = {}


def grid_of(oc, st):
    k = (st.n, st.W, st.H, st.seed)
    if k not in _grids:
        g = oc.synthetic_lf(st.n, st.W, st.H, st.seed)
        g.setflags(write=False)
        _grids[k] = g
    return _grids[k]


def shadow(oc, st):
    shape = iw.Shape(f"g{st.cols}x{st.rows}_{st.W}x{st.H}", st.cols, st.rows, st.W, st.H, st.ids, (4, 2))
    return iw.Shadow(shape, grid_of(oc, st), focus=st.focus, rng=st.rng, radius=st.radius, steps=st.steps, layout=st.layout, siting=st.siting[0],
                     released=st.inputs == "released", views=st.V, wide=st.wide)


def held(oc, st):
    """the input rows a windowed state holds: those its fixed-focus offsets sample, as tests/dispatch_windows.py sizes them"""
    return L.input_rows(st.band, shadow(oc, st).params(L).focused_offsets, st.H)


# ---- a context and the calls that take it from state to state ----------------------------------------------------------------------------------------

class Run:
    def __init__(self, ctx):
        self.ctx, self.state, self.keep, self.log = ctx, None, [], []


def _device(run, what, array):
    """a caller's device buffer (a torch tensor: 256-byte aligned), kept alive with the Run"""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(array)).to("cuda:0")
    torch.cuda.synchronize()   # torch's stream and the context's know nothing of each other
    run.keep.append(t)         # never freed while the context lives
    return t.data_ptr(), t.numel() * t.element_size()


def _call(run, name, *args, **kw):
    run.log.append(name)
    return getattr(run.ctx, name)(*args, **kw)


def set_variants(run, st):
    for method, name in zip(("STD", "TEN_WM"), st.variant):
        _call(run, "set_variant", method, name)


def set_rows(oc, run, st):
    s = shadow(oc, st)
    D, O = iw._view_offsets(L, s)
    if st.rows_kind == "int":
        _call(run, "set_view_offsets", D)
    else:
        _call(run, "set_view_float_offsets", O)
        if st.rows_kind == "view_maps":
            _call(run, "view_focus_maps", s.view_ids(L))


def move(oc, run, after, again=None, on_grid=None):
    """the calls that take run.ctx from run.state (None: a context fresh from lfi_create) to `after`.  again: "grid" / "params" — the call is
    made although nothing it takes differs.  on_grid(): called right after lfi_set_grid, before anything is uploaded or set."""
    ctx, b = run.ctx, run.state
    fresh = b is None
    prev = b if not fresh else State(0, 0, 0, 0)     # the settings of a new context
    s = shadow(oc, after)
    grid = fresh or again == "grid" or b.dims != after.dims
    if grid:
        _call(run, "set_grid", *after.dims)
        if on_grid:
            on_grid()
    window = after.window != (None if grid else b.window)
    if window:
        assert after.window is not None, "a row window goes with lfi_set_grid only"
        _call(run, "set_row_window", *after.window, *held(oc, after))
    planes = grid or window                          # new input planes: the parameters, the views and the kept set went with the old ones
    # context settings: lfi_set_grid leaves them alone
    if after.layout != prev.layout:
        _call(run, "set_output_layout", after.layout)
    if after.steps != prev.steps:
        _call(run, "set_focus_steps", after.steps)
    if after.siting != prev.siting:
        _call(run, "set_yuv_siting", *after.siting)
    if after.variant != prev.variant:
        set_variants(run, after)
    if after.stream != prev.stream:
        if after.stream == "caller":
            import torch
            run.keep.append(torch.cuda.Stream())
            _call(run, "set_stream", run.keep[-1].cuda_stream)
        else:
            _call(run, "set_stream", None)
    # inputs
    was = "none" if planes else b.inputs
    new_images = not planes and b.seed != after.seed
    i0, i1 = held(oc, after) if after.windowed else (0, after.H)
    if after.inputs == "attached":
        if was != "attached" or new_images:
            _call(run, "attach_grid", *_device(run, "grid", s.grid[:, i0:i1]))
            _call(run, "grid_modified")
    elif was == "none" or new_images:
        _call(run, "upload_grid", s.grid)
    else:
        assert was == after.inputs or (was, after.inputs) == ("owned", "released"), f"{was} -> {after.inputs} needs lfi_set_grid"
    # parameters
    params = planes or again == "params" or b.params_key() != after.params_key()
    if params:
        _call(run, "set_params", s.params(L), after.flags)
    # views: an attached buffer is forgotten with the planes, the layout and a view count it does not hold
    freed = planes or after.layout != prev.layout or (params and prev.V != after.V and not prev.views >= after.V)
    if after.views and (freed or prev.views != after.views):
        assert after.views >= after.V
        nbytes = ctx.view_layout().view_stride_bytes * after.views
        _call(run, "attach_views", *_device(run, "views", np.zeros(nbytes, np.uint8)))
    else:
        assert after.views == (0 if freed else prev.views), "the state says attached views and no call attaches them"
    if after.inputs == "released" and was != "released":
        _call(run, "release_inputs")
    # per-view rows: lfi_set_params clears them
    if after.rows_kind:
        if params or b.rows_kind != after.rows_kind:
            set_rows(oc, run, after)
    elif not params and not fresh and b.rows_kind:
        _call(run, "set_view_offsets", None)
        _call(run, "set_view_float_offsets", None)
    run.state = after


def memory(ctx):
    mi = ctx.memory_info()
    return {name: getattr(mi, name) for name, _ in mi._fields_ if name.endswith("_bytes")}


def refused(run, message, call):
    """call() must raise LfiError with `message` and leave lfi_memory_info as it was"""
    before = memory(run.ctx)
    try:
        call()
    except L.LfiError as e:
        assert message in str(e), ("refused with another message", message, str(e))
    else:
        raise AssertionError(("served where include/lfi.h refuses", message))
    assert memory(run.ctx) == before, ("the refused call changed lfi_memory_info", before, memory(run.ctx))


# ---- probes -------------------------------------------------------------------------------------------------------------------------------------

RUN = ("run", None)
W_COVER = "the input row window does not cover"
W_FOCUS = "does not work on a row window"
RELEASED = "the RGBA inputs were released"
NEEDS_PLANAR = "the RGBA view layout is not supported"
ROWS_STATE = "the state's per-view rows replace the parameters' offsets: state_rows holds this state"
FLAGGED = "the flagged renders are held by the flag's own probes"


def SKIP(reason):
    return ("skip", reason)


def REFUSED(message):
    return ("refused", message)


def _band(a, st):
    return a[:, st.band[0]:st.band[1]]


def _outside_zero(a, st):
    o0, o1 = st.band
    assert not a[:, :o0].any() and not a[:, o1:].any(), "rows outside the band were downloaded"


def _fixed_mode(st, released_ok=True):
    """what a plain fixed-focus render meets in the state"""
    if st.rows_kind:
        return SKIP(ROWS_STATE)
    if st.flags & VIEW_FLAGS and st.layout != "planar":
        return REFUSED(NEEDS_PLANAR)
    if st.inputs == "released" and not released_ok:
        return REFUSED(RELEASED)
    return RUN


class Probe:
    name = ""
    calls = ()         # the functions of include/lfi.h the probe calls
    colour = True      # its expected output is colour bytes: two states must differ in half of them (else: in any element)

    fields = ("dims", "V", "focus", "wide", "seed", "band")   # the state's fields the expected output depends on

    def mode(self, st):
        return RUN

    def depends(self, st):
        return tuple(getattr(st, f) for f in self.fields)

    def flat(self, want):
        return [np.asarray(w) for w in (want if isinstance(want, (list, tuple)) else [want])]

    def compared(self, want, st):
        """the expected output as the bytes two states are compared in: a colour probe's colour bytes of the state's band"""
        return np.concatenate([(_band(f, st) if f.ndim == 4 else f)[..., :3].ravel() for f in self.flat(want)])

    def bytes(self, got):
        """what a reused context must give byte for byte as a fresh one does"""
        return [np.asarray(g) for g in (got if isinstance(got, (list, tuple)) else [got]) if isinstance(g, np.ndarray)]

    def refuse(self, oc, run, st, message):
        refused(run, message, lambda: self.read(oc, run, st))


class FromReader(Probe):
    """a reader of tests/input_writers.py: its oracle, its call and its check, in the view layout and under the variants the state left"""

    def __init__(self, reader, calls, colour=True, fields=None):
        self.reader, self.name, self.calls, self.colour = reader, reader.name, calls, colour
        if fields:
            self.fields = fields

    def want(self, oc, st, run=None):
        return self.reader.want(oc, L, shadow(oc, st), run.ctx if run and self.reader.name == "download_derived" else None)

    def read(self, oc, run, st):
        s = shadow(oc, st)
        self.reader.prepare(L, run.ctx, s, fixed=False)
        try:
            return self.reader.read(L, run.ctx, s)
        finally:
            self.reader.done(run.ctx)
            if st.variant != AUTO:     # the readers of input_writers set "auto" themselves: back to what the state says
                for method, name in zip(("STD", "TEN_WM"), st.variant):
                    run.ctx.set_variant(method, name)

    def check(self, got, want, st):
        self.reader.check(got, want)

    def flat(self, want):
        return self.reader.flat(want)


class Std(FromReader):
    def __init__(self):
        super().__init__(iw.Std(), ("lfi_render", "lfi_download_view", "lfi_set_variant", "lfi_debug_poison"))
        self.name = "std"

    def mode(self, st):
        return _fixed_mode(st)

    def depends(self, st):
        return super().depends(st) + (st.flags & (IN_FRAME | LINEAR),)

    def read(self, oc, run, st):
        """by whatever STD variant the context holds: no lfi_set_variant here"""
        run.ctx.poison(L.LFI_POISON_VIEWS, iw._byte())
        run.ctx.render("STD")
        if st.variant[0] != "auto" and not st.flags & VIEW_FLAGS:
            assert run.ctx.last_kernel_name() == KERNEL_OF[st.variant[0]], ("the STD variant was lost", run.ctx.last_kernel_name())
        return run.ctx.download_views()

    def want(self, oc, st, run=None):
        if st.flags & IN_FRAME:
            return _cached("inframe_std", st, lambda: _rgba(_inframe(oc, st).bytes))
        if st.flags & LINEAR:
            return _cached("linear_std", st, lambda: _rgba(_linear(oc, st).bytes))
        return super().want(oc, st)

    def check(self, got, want, st):
        _outside_zero(got, st)
        self.reader.check(_band(got, st), _band(want, st))


class Ten(FromReader):
    def __init__(self):
        super().__init__(iw.TenPlanar(), ("lfi_render", "lfi_download_view", "lfi_set_variant", "lfi_debug_poison", "lfi_last_kernel_name"))
        self.name = "ten_wm"

    def mode(self, st):
        if st.flags & (VIEW_FLAGS | PER_BATCH):
            return SKIP(FLAGGED)
        return _fixed_mode(st)

    def read(self, oc, run, st):
        """by whatever TEN_WM variant the context holds: no lfi_set_variant here"""
        run.ctx.poison(L.LFI_POISON_VIEWS, iw._byte())
        run.ctx.render("TEN_WM")
        kernel = run.ctx.last_kernel_name()
        if st.variant[1] != "auto":
            assert kernel == ten_kernel_of(st), ("the TEN_WM variant was lost", kernel, ten_kernel_of(st))
        return run.ctx.download_views(), kernel

    def check(self, got, want, st):
        _outside_zero(got[0], st)
        self.reader.check((_band(got[0], st), got[1]), tuple(_band(w, st) for w in want))


class StdVariant(Std):
    """the same render by another kernel (lfi_set_variant): persist_m2_nt honours a row window"""

    def __init__(self):
        super().__init__()
        self.name = "std_variant_persist"

    def mode(self, st):
        if st.inputs == "released":
            return SKIP("the variant's kernel is not one of those the planar copy alone serves")
        return SKIP(FLAGGED) if st.flags & VIEW_FLAGS else _fixed_mode(st)

    def read(self, oc, run, st):
        run.ctx.poison(L.LFI_POISON_VIEWS, iw._byte())
        run.ctx.set_variant("STD", "persist_m2_nt")
        try:
            run.ctx.render("STD")
            return run.ctx.download_views()
        finally:
            run.ctx.set_variant("STD", st.variant[0])


class SubRange(Std):
    """views [1, V − 1) under poison: the views outside the range keep the poison"""

    def __init__(self):
        super().__init__()
        self.name = "std_view_range"

    def want(self, oc, st, run=None):
        return super().want(oc, st)[1:st.V - 1]

    def read(self, oc, run, st):
        return poison.render_range(run.ctx, "STD", 1, st.V - 1)


class ViewRowsProbe(FromReader):
    def __init__(self):
        super().__init__(iw.ViewRows(), ("lfi_set_view_offsets", "lfi_render", "lfi_download_view", "lfi_last_kernel_name", "lfi_debug_poison"),
                         fields=("dims", "V", "wide", "seed", "band"))     # its offsets come from its own focus ramp, not from the parameters' focus

    def mode(self, st):
        if st.rows_kind:
            return SKIP(ROWS_STATE)
        if st.windowed:
            return SKIP("the ramp's rows reach beyond the rows the window holds; tests/view_rows.py has windowed rows")
        if st.inputs == "released":
            return SKIP("served or refused by the copy's padding, which the history of the context decides; tests/view_rows.py holds both")
        if st.flags & VIEW_FLAGS:
            return REFUSED("per-view rows (lfi_set_view_offsets, lfi_set_view_float_offsets) are not supported")
        if st.flags & PER_BATCH:
            return REFUSED("LFI_FLAG_TEN_ROUND_PER_BATCH is not supported")
        return RUN


class AllFocusProbe(FromReader):
    def __init__(self, reader=None, calls=("lfi_upload_map", "lfi_render", "lfi_download_view", "lfi_set_variant", "lfi_debug_poison")):
        super().__init__(reader or iw.AllFocus(), calls, fields=Probe.fields + ("rng",))

    def mode(self, st):
        if st.rows_kind:
            return SKIP(ROWS_STATE)
        if st.flags & VIEW_FLAGS:       # asked first: launch_blend turns to the flagged route before anything else
            return REFUSED("all-focus renders are not supported")
        if st.inputs == "released":
            return REFUSED(RELEASED)
        if st.windowed:
            return REFUSED(W_COVER)
        return RUN


class _TenAllFocus(iw.Reader):
    name = "all_focus_ten_wm_uploaded_map"

    def want(self, oc, L_, s, ctx=None):
        hp, m = s.params(L), iw._the_map(s.shape)
        kw = dict(all_focus=True, map_plane=m, focus=hp.focus, rng=hp.range, threads=8)

        def compute():
            lo, hi = ten_interval.bounds(oc, s.grid, hp, **kw)
            return oc.blend_ten(s.grid, hp.focused_offsets, hp.offsets, hp.weights, model=oc.TEN_M16, **kw), lo, hi
        return iw._cached("ten_af", s, compute)

    def prepare(self, L_, ctx, s, fixed=True):
        ctx.set_variant("TEN_WM", "auto")
        for k in (0, 1):
            ctx.upload_map(k, iw._the_map(s.shape))
        ctx.poison(L.LFI_POISON_VIEWS, iw._byte())

    def read(self, L_, ctx, s):
        ctx.render("TEN_WM", all_focus=True)
        return ctx.download_views(), ctx.last_kernel_name()

    check = iw.TenPlanar.check
    flat = iw.TenPlanar.flat


class TenAllFocus(AllFocusProbe):
    def __init__(self):
        super().__init__(_TenAllFocus(), ("lfi_upload_map", "lfi_render", "lfi_download_view", "lfi_set_variant", "lfi_debug_poison", "lfi_last_kernel_name"))

    def mode(self, st):
        return SKIP(FLAGGED) if st.flags & PER_BATCH else super().mode(st)


class FocusProbe(FromReader):
    """the readers that sample the focus ids: refused without the RGBA planes; lfi_focus_map computes a band, the others refuse a window"""

    def __init__(self, reader, calls, band_message, fields):
        super().__init__(reader, calls, colour=False, fields=fields)
        self.band_message = band_message

    def compared(self, want, st):
        return np.concatenate([f.ravel().view(np.uint8) for f in self.flat(want)])

    def mode(self, st):
        if st.inputs == "released":
            return REFUSED(RELEASED)
        if st.windowed:
            return REFUSED(self.band_message)
        if self.reader.variant == "plain" and st.steps != 32:
            return REFUSED("computes 32 candidates only")
        if self.reader.name == "view_focus_maps_then_focus_map" and st.rows_kind:
            return SKIP(ROWS_STATE)
        return RUN


class DerivedProbe(FromReader):
    def __init__(self):
        super().__init__(iw.Derived(), ("lfi_debug_derived_layout", "lfi_debug_download_derived"), colour=False)

    def mode(self, st):
        return RUN if st.inputs == "released" else SKIP("serves a current copy only, and whether it is current is what the renders show (input_writers.readers_of)")


_wants = {}


def _cached(kind, st, fn):
    k = (kind,) + st.want_key()
    if k not in _wants:
        _wants[k] = fn()
    return _wants[k]


def _rgba(rgb):
    out = np.full(rgb.shape[:-1] + (4,), 255, np.uint8)
    out[..., :3] = rgb
    return out


def _inframe(oc, st):
    s = shadow(oc, st)
    return _cached("inframe", st, lambda: inframe_ref.restate(s.grid, s.params(L)))


def _linear(oc, st):
    s = shadow(oc, st)
    return _cached("linear", st, lambda: linear_ref.restate(s.grid, s.params(L)))


class StateRows(Probe):
    """a state with per-view rows set: integer rows — a fixed-focus STD render from each view's own offsets; float rows — an all-focus STD
    render from each view's own float offsets and the uploaded map, or (view_maps) each view's own estimated map"""
    name = "state_rows"

    def counterpart(self, st):
        """the probe whose answer a context that ignored the rows would give"""
        return "std" if st.rows_kind == "int" else "all_focus_std_uploaded_map"
    fields = Probe.fields + ("rng", "rows_kind", "radius", "ids")
    calls = ("lfi_render", "lfi_download_view", "lfi_upload_map", "lfi_debug_poison", "lfi_last_kernel_name")

    def mode(self, st):
        return RUN if st.rows_kind else SKIP("no per-view rows in the state")

    def want(self, oc, st, run=None):
        s = shadow(oc, st)
        if st.rows_kind == "int":
            return iw.ViewRows().want(oc, L, s)
        hp, O = s.params(L), iw._view_offsets(L, s)[1]

        def compute():
            out = []
            for v in range(st.V):
                m = iw._the_map(s.shape)
                if st.rows_kind == "view_maps":
                    m = iw._want_maps(oc, L, s, np.ascontiguousarray(O[v]), np.ascontiguousarray(s.view_ids(L)[v]), 32)[1]
                out.append(oc.blend_std(s.grid, hp.focused_offsets, np.ascontiguousarray(O[v]), hp.weights[v:v + 1], all_focus=True, map_plane=m, focus=hp.focus,
                                        rng=hp.range)[0])
            return np.stack(out)
        return _cached("state_rows", st, compute)

    def read(self, oc, run, st):
        ctx = run.ctx
        if st.rows_kind == "float":
            for k in (0, 1):
                ctx.upload_map(k, iw._the_map(shadow(oc, st).shape))
        ctx.poison(L.LFI_POISON_VIEWS, iw._byte())
        ctx.render("STD", all_focus=st.rows_kind != "int")
        return ctx.download_views(), ctx.last_kernel_name()

    def check(self, got, want, st):
        views, kernel = got
        assert kernel.startswith("blend_vfocus"), kernel
        assert ("view_maps" in kernel) == (st.rows_kind == "view_maps") and ("_af" in kernel) == (st.rows_kind != "int"), (kernel, st.rows_kind)
        assert (views == want).all(), ("per-view rows of the state", st.rows_kind, int((views != want).sum()))

    def flat(self, want):
        return [want]


class DeepProbe(Probe):
    """LFI_FLAG_DEEP_VIEWS: STD codes and bytes == the oracle's; TEN_WM codes inside the interval of the exact sum with two more bits, and
    code >> 2 the byte of the same launch (tests/test_gpu_deep.py's contract)"""
    name = "deep_views"
    calls = ("lfi_prepare", "lfi_render", "lfi_download_views_yuv", "lfi_download_view", "lfi_debug_poison", "lfi_sync")

    def mode(self, st):
        return RUN if st.flags & DEEP and st.layout == "planar" else SKIP("LFI_FLAG_DEEP_VIEWS is not set, or std holds its refusal of the RGBA layout")

    def want(self, oc, st, run=None):
        s = shadow(oc, st)
        hp = s.params(L)

        def compute():
            out, pre = oc.blend_std(s.grid, hp.focused_offsets, hp.offsets, hp.weights, return_prequant=True)
            S, eps = ten_interval.exact_sums(oc, s.grid, hp)
            return (out, deep_ref.q10_std(pre)) + tuple(deep_ref.interval10(S, eps))
        return _cached("deep", st, compute)

    def read(self, oc, run, st):
        ctx, out = run.ctx, []
        for method in ("STD", "TEN_WM"):
            ctx.prepare(method)      # allocates the deep planes
            ctx.poison(poison.RENDER | L.LFI_POISON_DEEP, iw._byte())
            ctx.render(method)
            ctx.sync()
            out += [ctx.download_deep_views(), ctx.download_views()]
        return out

    def check(self, got, want, st):
        (deep_s, views_s, deep_t, views_t), (std, codes, lo, hi) = got, want
        assert (deep_s == codes).all() and (views_s == std).all(), ("deep STD", int((deep_s != codes).sum()), int((views_s != std).sum()))
        outside = int(((deep_t < lo) | (deep_t > hi)).sum())
        assert outside == 0, ("deep TEN_WM codes outside their interval", outside)
        assert (deep_t >> 2 == views_t[..., :3]).all() and (views_t[..., 3] == 255).all()

    def flat(self, want):
        return [want[0]]


class InFrameTen(Probe):
    """LFI_FLAG_IN_FRAME, TEN_WM: inside inframe_ref.ten_interval_of; 0 where no image has the pixel in frame (std holds the STD bytes)"""
    name = "inframe_ten_wm"
    calls = ("lfi_render", "lfi_download_view", "lfi_debug_poison")

    def mode(self, st):
        return RUN if st.flags & IN_FRAME and st.layout == "planar" else SKIP("LFI_FLAG_IN_FRAME is not set, or std holds its refusal of the RGBA layout")

    def want(self, oc, st, run=None):
        s = shadow(oc, st)
        res = _inframe(oc, st)
        return _cached("inframe_ten", st, lambda: inframe_ref.ten_interval_of(res, s.params(L), st.n) + (res.none_in,))

    def read(self, oc, run, st):
        poison.render(run.ctx, "TEN_WM")
        return run.ctx.download_views()

    def check(self, got, want, st):
        lo, hi, none_in = want
        out = ten_interval.outside(got, lo, hi)
        assert out == 0, ("in-frame TEN_WM bytes outside their interval", out)
        assert (got[:, none_in][..., :3] == 0).all()

    def flat(self, want):
        return [want[0]]


class LinearStd(Probe):
    """LFI_FLAG_LINEAR_LIGHT, STD: `==` linear_ref's restatement, by blend_linear; and the deep views of an earlier deep render are gone — a
    linear-light launch writes the views without their deep planes (the hand-over linear <-> deep)"""
    name = "linear_std"
    calls = ("lfi_render", "lfi_download_view", "lfi_debug_poison", "lfi_last_kernel_name", "lfi_download_views_yuv")
    method, kernel = "STD", "blend_linear<STD>"

    def counterpart(self, st):
        """the probe whose answer a context that ignored the flag would give"""
        return "std"

    def mode(self, st):
        return RUN if st.flags & LINEAR and st.layout == "planar" else SKIP("LFI_FLAG_LINEAR_LIGHT is not set, or std holds its refusal of the RGBA layout")

    def depends(self, st):
        return super().depends(st) + (st.flags & LINEAR,)

    def want(self, oc, st, run=None):
        return _rgba(_linear(oc, st).bytes)

    def read(self, oc, run, st):
        poison.render(run.ctx, self.method)
        kernel = run.ctx.last_kernel_name()
        refused(run, "LFI_YUV_DEEP", lambda: run.ctx.download_deep_views())
        return run.ctx.download_views(), kernel

    def check(self, got, want, st):
        views, kernel = got
        assert kernel == self.kernel, kernel
        assert (views == want).all(), ("linear-light STD", int((views != want).sum()))


class LinearTen(LinearStd):
    """LFI_FLAG_LINEAR_LIGHT, TEN_WM: inside linear_ref.ten_interval_of"""
    name = "linear_ten_wm"
    method, kernel = "TEN_WM", "blend_linear<TEN_WM>"

    def counterpart(self, st):
        return "ten_wm"

    def want(self, oc, st, run=None):
        s = shadow(oc, st)
        return _cached("linear_ten", st, lambda: linear_ref.ten_interval_of(_linear(oc, st), s.params(L), st.n))

    def check(self, got, want, st):
        views, kernel = got
        assert kernel == self.kernel, kernel
        out = ten_interval.outside(views, *want)
        assert out == 0, ("linear-light TEN_WM bytes outside their interval", out)

    def flat(self, want):
        return [want[0]]


class PerBatch(Probe):
    """LFI_FLAG_TEN_ROUND_PER_BATCH: the M16 model byte for byte"""
    name = "ten_wm_per_batch"
    calls = ("lfi_render", "lfi_download_view", "lfi_debug_poison")

    def mode(self, st):
        if not st.flags & PER_BATCH:
            return SKIP("LFI_FLAG_TEN_ROUND_PER_BATCH is not set")
        return _fixed_mode(st)

    def want(self, oc, st, run=None):
        return iw.TenPlanar().want(oc, L, shadow(oc, st))[0]

    def read(self, oc, run, st):
        poison.render(run.ctx, "TEN_WM")
        return run.ctx.download_views()

    def check(self, got, want, st):
        assert (got == want).all(), ("per-batch TEN_WM is not M16", int((got != want).sum()))


class RenderStream(Probe):
    """lfi_render_stream over the weight rows reversed, then as they are: 2·V views; the last block leaves the state's own weights behind"""
    name = "render_stream"
    calls = ("lfi_render_stream", "lfi_set_variant")

    def mode(self, st):
        if st.rows_kind:
            return SKIP(ROWS_STATE)
        if st.flags & VIEW_FLAGS:
            return REFUSED("lfi_render_stream is not supported")
        if st.layout != "rgba":
            return REFUSED("downloads need the RGBA view layout")
        return RUN

    def want(self, oc, st, run=None):
        std = iw.Std().want(oc, L, shadow(oc, st))
        return np.concatenate([std[::-1], std])

    def read(self, oc, run, st):
        w = shadow(oc, st).params(L).weights
        out = poison.sentinel((2 * st.V, st.H, st.W, 4))
        run.ctx.render_stream("STD", np.concatenate([w[::-1], w]), out)
        return out

    def check(self, got, want, st):
        o0, o1 = st.band
        assert (got[:, :o0] == poison.SENTINEL).all() and (got[:, o1:] == poison.SENTINEL).all(), "rows outside the band were written"
        assert (_band(got, st) == _band(want, st)).all(), ("render_stream", int((_band(got, st) != _band(want, st)).sum()))


def _records(recs, n, agg):
    return np.frombuffer(ctypes.string_at(recs, ctypes.sizeof(L.ViewQuality) * n) + ctypes.string_at(ctypes.byref(agg), ctypes.sizeof(agg)), np.uint8).copy()


def _same(x, y, tol, relative):
    if np.isinf(x) or np.isinf(y):
        return x == y
    return abs(x - y) <= (tol * abs(y) if relative else tol)


def check_quality(q, want, where):
    """as tests/test_gpu_compare_views.py::_check_quality: the MSE exactly, SSIM to rtol 1e-9, PSNR to 1e-9 dB"""
    for c in range(3):
        assert q.mse[c] == want["mse"][c], (where, "mse", c, q.mse[c], want["mse"][c])
        assert _same(q.ssim[c], want["ssim"][c], 1e-9, True), (where, "ssim", c, q.ssim[c], want["ssim"][c])
        assert _same(q.psnr[c], want["psnr"][c], 1e-9, False), (where, "psnr", c, q.psnr[c], want["psnr"][c])
    assert _same(q.ssim_all, want["ssim_all"], 1e-9, True), (where, "ssim_all", q.ssim_all, want["ssim_all"])
    assert _same(q.psnr_all, want["psnr_all"], 1e-9, False), (where, "psnr_all", q.psnr_all, want["psnr_all"])


class KeepCompare(Probe):
    """STD rendered and kept (lfi_keep_views), TEN_WM rendered and compared with the kept set (lfi_compare_views): the kept views are the
    oracle's STD, the records tests/quality_ref.py's on the two downloads"""
    name = "keep_and_compare_views"
    calls = ("lfi_keep_views", "lfi_compare_views", "lfi_render", "lfi_download_view", "lfi_debug_poison", "lfi_sync")

    def mode(self, st):
        if st.flags & (VIEW_FLAGS | PER_BATCH):
            return SKIP(FLAGGED)
        if st.rows_kind:
            return SKIP(ROWS_STATE)
        if st.windowed:
            return REFUSED("lfi_compare_views needs whole views (no row window)")
        return RUN

    def want(self, oc, st, run=None):
        return iw.Std().want(oc, L, shadow(oc, st))

    def read(self, oc, run, st):
        ctx = run.ctx
        poison.render(ctx, "STD")
        ctx.keep_views()
        std = ctx.download_views()
        poison.render(ctx, "TEN_WM")
        ten = ctx.download_views()
        try:
            recs, agg = ctx.compare_views()
        finally:
            ctx.drop_kept_views()
        return std, ten, _records(recs, st.V, agg), (recs, agg)

    def check(self, got, want, st):
        std, ten, _, (recs, agg) = got
        assert (std == want).all(), ("the kept STD views", int((std != want).sum()))
        per_view = [quality_ref.compare(ten[k], std[k]) for k in range(st.V)]
        for k, w in enumerate(per_view):
            r = recs[k]
            assert list(r.sq_err) == w["sq_err"], (k, list(r.sq_err), w["sq_err"])
            assert (r.differing_bytes, r.windows, r.max_abs_diff) == (w["differing_bytes"], w["windows"], w["max_abs_diff"]), k
            check_quality(r.q, w, k)
        check_quality(agg, quality_ref.aggregate(per_view, st.W, st.H), "all")

    def bytes(self, got):
        return list(got[:3])

    def refuse(self, oc, run, st, message):
        poison.render(run.ctx, "STD")
        run.ctx.keep_views()         # a window's band is kept as the views hold it; the compare is what a window refuses
        try:
            refused(run, message, lambda: run.ctx.compare_views())
        finally:
            run.ctx.drop_kept_views()


class OutputProbe(Probe):
    """an output call after an STD render under poison: the views' own download is the oracle's, and the call's output is its restatement
    applied to that download"""
    refusal = None     # under a row window

    def mode(self, st):
        if st.flags & VIEW_FLAGS:
            return SKIP(FLAGGED)
        if st.rows_kind:
            return SKIP(ROWS_STATE)
        if st.windowed:
            return REFUSED(self.refusal) if self.refusal else SKIP("a band's rows of this output: its own test file has windowed cases")
        return RUN

    def want(self, oc, st, run=None):
        views = iw.Std().want(oc, L, shadow(oc, st))
        return views, _cached(self.name, st, lambda: self.restate(views, st))

    def read(self, oc, run, st):
        poison.render(run.ctx, "STD")
        views = run.ctx.download_views()
        return views, self.output(run.ctx, st)

    def refuse(self, oc, run, st, message):
        poison.render(run.ctx, "STD")
        refused(run, message, lambda: self.output(run.ctx, st))

    def check(self, got, want, st):
        views, out = got
        assert (views == want[0]).all(), (self.name, "the views", int((views != want[0]).sum()))
        ref = self.restate(views, st)   # on the views' own download
        assert out.shape == ref.shape and (out == ref).all(), (self.name, int((out != ref).sum()))

    def compared(self, want, st):
        return want[1][..., :3].ravel()


class QuiltTiles(OutputProbe):
    name = "download_quilt_tiles_two_parts"
    calls = ("lfi_download_quilt_tiles", "lfi_render", "lfi_download_view", "lfi_debug_poison", "lfi_sync")

    def output(self, ctx, st):
        quilt = poison.sentinel((2 * st.H, 2 * st.W, 4))
        ctx.download_quilt_tiles(quilt, 2, 2, 0, 3)
        ctx.download_quilt_tiles(quilt, 2, 2, 3, 1, v0=3)
        return quilt

    def restate(self, views, st):
        return views[:4].reshape(2, 2, st.H, st.W, 4).transpose(0, 2, 1, 3, 4).reshape(2 * st.H, 2 * st.W, 4)


def tile_size(st):
    """a third of the width and half the height: follows the state's size"""
    return max(st.W // 3, 1), max(st.H // 2, 1)


class QuiltScaled(OutputProbe):
    name = "download_quilt_scaled"
    calls = ("lfi_download_quilt_scaled", "lfi_render", "lfi_download_view", "lfi_debug_poison", "lfi_sync")
    refusal = "a scaled quilt needs whole views"

    def output(self, ctx, st):
        return ctx.download_quilt_scaled(2, 2, *tile_size(st))

    def restate(self, views, st):
        return scaled_quilt_ref.quilt(views[:4], 2, 2, *tile_size(st))


class Yuv420(OutputProbe):
    name = "download_views_yuv420"
    calls = ("lfi_download_views_yuv420", "lfi_render", "lfi_download_view", "lfi_debug_poison", "lfi_sync")
    refusal = "YUV 4:2:0 frames need whole views"
    fields = Probe.fields + ("siting_out",)

    def compared(self, want, st):
        return want[1][:, st.W * st.H:].ravel()      # the chroma planes: the luma does not read the siting

    def output(self, ctx, st):
        return ctx.download_views_yuv420(matrix="601", range="full")

    def restate(self, views, st):
        ref = yuv_left_ref if st.siting[1] == "left" else yuv_ref
        return ref.frames(views, yuv_ref.BT601, yuv_ref.FULL)



def _left(st):
    return st.siting[1] == "left"


class ViewsYuv(OutputProbe):
    """lfi_download_views_yuv into host surfaces: I420 tight, NV12 pitched, P010 tight (the deep formats: deep_views)"""
    calls = ("lfi_download_views_yuv", "lfi_render", "lfi_download_view", "lfi_debug_poison", "lfi_sync")
    refusal = "YUV 4:2:0 frames need whole views"
    fields = Probe.fields + ("siting_out",)

    def __init__(self, fmt):
        self.fmt, self.name = fmt, "download_views_yuv_" + fmt

    def output(self, ctx, st):
        if self.fmt == "p010":
            lay = yuv10_ref.tight(yuv10_ref.P010, st.W, st.H)
            arr = np.full((st.V, lay.frame_stride), 0x11, np.uint8)
            ctx.download_views_yuv(yuv10_ref.descriptor(L, lay, yuv10_ref.HOST, arr.ctypes.data, keep=arr))
            return yuv10_ref.gather(arr, lay)
        lay = sref.tight(sref.I420, st.W, st.H) if self.fmt == "i420" else sref.pitched(sref.NV12, st.W, st.H)
        arr = np.full((st.V, lay.frame_stride), 0x11, np.uint8)
        ctx.download_views_yuv(sref.descriptor(L, lay, sref.HOST, arr.ctypes.data, keep=arr))
        assert sref.padding_holds(arr, lay, 0x11), "bytes outside the planes were written"
        return sref.gather(arr, lay)

    def restate(self, views, st):
        if self.fmt == "p010":
            return yuv10_ref.words(yuv10_ref.frames(views, yuv10_ref.BT709, yuv10_ref.LIMITED, yuv10_ref.LEFT if _left(st) else yuv10_ref.CENTRE), yuv10_ref.P010)
        return (yuv_left_ref if _left(st) else yuv_ref).frames(views, yuv_ref.BT709, yuv_ref.LIMITED)

    def compared(self, want, st):
        return want[1][:, st.W * st.H:].ravel()      # the chroma samples: the luma does not read the siting


class QuiltYuv(OutputProbe):
    name = "download_quilt_yuv"
    calls = ("lfi_download_quilt_yuv", "lfi_render", "lfi_download_view", "lfi_debug_poison", "lfi_sync")
    refusal = "a scaled quilt needs whole views"
    fields = Probe.fields + ("siting_out",)

    def output(self, ctx, st):
        tw, th = tile_size(st)
        lay = sref.tight(sref.I420, 2 * tw, 2 * th)
        arr = np.full((1, lay.frame_stride), 0x11, np.uint8)
        ctx.download_quilt_yuv(2, 2, 1, tw, th, "601", "full", sref.descriptor(L, lay, sref.HOST, arr.ctypes.data, keep=arr))
        return sref.gather(arr, lay)

    def restate(self, views, st):
        quilt = scaled_quilt_ref.quilt(views[1:5], 2, 2, *tile_size(st))     # views 1 … 4: view 0 is the trajectory's start whatever the view count
        return (yuv_left_ref if _left(st) else yuv_ref).frame(quilt, yuv_ref.BT601, yuv_ref.FULL)[None]

    def compared(self, want, st):
        tw, th = tile_size(st)
        return want[1][:, 4 * tw * th:].ravel()      # the chroma samples


def even_tile(st):
    return max(st.W // 3 & ~1, 2), max(st.H // 2 & ~1, 2)


class RgbdYuv(OutputProbe):
    """views 1 and 2 beside the uploaded map 1"""
    name = "download_rgbd_yuv"
    calls = ("lfi_download_rgbd_yuv", "lfi_upload_map", "lfi_render", "lfi_download_view", "lfi_debug_poison", "lfi_sync")

    def mode(self, st):
        if _left(st):
            return SKIP("lfi_download_rgbd_yuv refuses left-sited output; tests/test_gpu_yuv_left.py holds the refusal")
        if st.windowed:
            return SKIP("the refusal of a window is download_quilt_yuv's; its order against the other refusals: tests/test_gpu_rgbd_yuv.py")
        return super().mode(st)

    def output(self, ctx, st):
        tw, th = even_tile(st)
        ctx.upload_map(1, iw._the_map(st))
        lay = sref.tight(sref.I420, 2 * tw, th)
        arr = np.full((2, lay.frame_stride), 0x11, np.uint8)
        ctx.download_rgbd_yuv(1, 2, 1, 0, tw, th, "709", "limited", sref.descriptor(L, lay, sref.HOST, arr.ctypes.data, keep=arr))
        return sref.gather(arr, lay)

    def restate(self, views, st):
        tw, th = even_tile(st)
        return np.stack([rgbd_yuv_ref.frame(views[v], iw._the_map(st), tw, th, False, yuv_ref.BT709, yuv_ref.LIMITED) for v in (1, 2)])

    def compared(self, want, st):
        return want[0][1:3, ..., :3].ravel()     # the two views the frames show: the depth side is the uploaded map in every state


def native_size(st):
    return st.W // 2 + 3, st.H - 5


class Native(OutputProbe):
    """lfi_download_native of views 1 … 4 through scaled tiles: plain (native_ref) and filtered (bilinear tiles, blended views, native_filter_ref)"""
    calls = ("lfi_download_native", "lfi_render", "lfi_download_view", "lfi_debug_poison", "lfi_sync")
    refusal = "a native image needs whole views"

    def __init__(self, filtered):
        self.filtered, self.name = filtered, "download_native_filtered" if filtered else "download_native"
        self.lens = native_ref.Lens(*native_ref.STEPS["slant"], 4, native_filter_ref.BILINEAR | native_filter_ref.BLEND if filtered else 0)

    def output(self, ctx, st):
        ctx.poison(L.LFI_POISON_SCRATCH, iw._byte())
        lens = self.lens
        return ctx.download_native(L.Lenticular(lens.x_step, lens.y_step, lens.phase0, lens.views, lens.flags), *native_size(st), *tile_size(st), v0=1)

    def restate(self, views, st):
        return (native_filter_ref if self.filtered else native_ref).native(views, self.lens, 1, *native_size(st), *tile_size(st))


class YuvUpload(Probe):
    """the input side: lfi_upload_images_yuv of I420 frames from host surfaces into the first and the last two images (the staging buffer yuv_in,
    sized by W and H, and the context's input siting), an STD render against the oracle on the images the restatement expands, then the
    state's own images back (lfi_upload_image)"""
    name = "upload_images_yuv_then_std"
    calls = ("lfi_upload_images_yuv", "lfi_render", "lfi_download_view", "lfi_debug_poison", "lfi_sync")
    fields = Probe.fields + ("siting_in",)
    writer = next(w for w in iw.WRITERS if w.name == "upload_images_yuv_i420_host")

    def mode(self, st):
        if st.flags & VIEW_FLAGS:
            return SKIP(FLAGGED)
        if st.rows_kind:
            return SKIP(ROWS_STATE)
        if st.inputs != "owned":
            return SKIP("the probe puts the state's images back with lfi_upload_image, into planes the context owns; tests/input_writers.py holds the writers of attached and released inputs")
        if st.windowed:
            return REFUSED("YUV 4:2:0 frames need whole images")
        return RUN

    def _write(self, oc, st):
        s = shadow(oc, st)
        env = iw.Env(L, oc, s.shape, 7, st.siting[0], s.params(L))
        return s, env, self.writer.make(env)

    def want(self, oc, st, run=None):
        def compute():
            s, env, payload = self._write(oc, st)
            return iw.Std().want(oc, L, replace(s, grid=iw.shadow_apply(s.grid, payload, self.writer)))
        return _cached(self.name, st, compute)

    def read(self, oc, run, st):
        s, env, payload = self._write(oc, st)
        keep = []
        try:
            self.writer.apply(L, run.ctx, payload, env, keep)
            poison.render(run.ctx, "STD")
            return run.ctx.download_views()
        finally:
            if st.band == (0, st.H):
                run.ctx.upload_grid(s.grid)

    def check(self, got, want, st):
        assert (got == want).all(), ("STD after the YUV upload", int((got != want).sum()), np.argwhere((got != want).any(axis=(1, 2, 3))).ravel().tolist())


_R = {r.name: r for r in iw.READERS}
_FOCUS = ("lfi_focus_map", "lfi_download_map", "lfi_set_variant", "lfi_debug_poison")
_F32 = ("dims", "focus", "rng", "radius", "ids", "seed")      # the estimate at 32 candidates
_FMAP = _F32 + ("steps",)
PROBES = [
    Std(), Ten(), StdVariant(), SubRange(), ViewRowsProbe(), AllFocusProbe(), TenAllFocus(),
    FocusProbe(_R["focus_map_factored"], _FOCUS, W_COVER, _FMAP), FocusProbe(_R["focus_map_factored_direct"], _FOCUS, W_COVER, _FMAP),
    FocusProbe(_R["focus_map_plain"], _FOCUS, W_COVER, _FMAP),
    FocusProbe(_R["view_focus_maps_then_focus_map"], _FOCUS + ("lfi_set_view_float_offsets", "lfi_view_focus_maps", "lfi_download_view_map"), W_FOCUS, _FMAP + ("V",)),
    FocusProbe(_R["focus_tiles_3x2"], ("lfi_focus_tiles",), W_FOCUS, _F32), FocusProbe(_R["focus_curve_rectangle"], ("lfi_focus_curve",), W_FOCUS, _F32),
    DerivedProbe(), StateRows(), DeepProbe(), InFrameTen(), LinearStd(), LinearTen(), PerBatch(), RenderStream(), KeepCompare(), QuiltTiles(), QuiltScaled(), Yuv420(),
    ViewsYuv("i420"), ViewsYuv("nv12"), ViewsYuv("p010"), QuiltYuv(), RgbdYuv(), Native(False), Native(True), YuvUpload(),
]
assert len({p.name for p in PROBES}) == len(PROBES)


def probes_of(st):
    """[(probe, kind, detail)] — every probe, with what it does in the state"""
    return [(p,) + p.mode(st) for p in PROBES]


def run_probe(oc, run, st, p, kind, detail, where):
    """one probe on the context, checked; returns what a fresh context must give byte for byte (None: refused or skipped)"""
    try:
        if kind == "refused":
            p.refuse(oc, run, st, detail)
            return None
        if kind == "skip":
            return None
        got = p.read(oc, run, st)
        p.check(got, p.want(oc, st, run), st)
        return p.bytes(got)
    except AssertionError as e:
        raise AssertionError(f"{where}: {p.name}: {e}") from None
    except L.LfiError as e:
        raise AssertionError(f"{where}: {p.name}: refused where include/lfi.h serves: {e}") from None


def run_probes(oc, run, st, where, only=None):
    return {p.name: run_probe(oc, run, st, p, kind, detail, where) for p, kind, detail in probes_of(st) if only is None or p.name in only}


# what every reading family answers on a context that has a grid and no parameters: each must be refused (lfi_set_grid again)
BARE = {
    "lfi_render": lambda ctx: ctx.render("STD"),
    "lfi_render all-focus": lambda ctx: ctx.render("TEN_WM", all_focus=True),
    "lfi_focus_map": lambda ctx: ctx.focus_map(),
    "lfi_focus_tiles": lambda ctx: ctx.focus_tiles(*iw.TILES),
    "lfi_focus_curve": lambda ctx: ctx.focus_curve(0, 0, 8, 8),
    "lfi_set_view_offsets": lambda ctx: ctx.set_view_offsets(np.zeros((1, ctx.n_images, 2), np.int32)),
    "lfi_set_view_float_offsets": lambda ctx: ctx.set_view_float_offsets(np.zeros((1, ctx.n_images, 2), np.float32)),
    "lfi_view_focus_maps": lambda ctx: ctx.view_focus_maps(np.zeros((1, 1), np.int32)),
    "lfi_download_view": lambda ctx: ctx.download_view(0),
    "lfi_download_view_map": lambda ctx: ctx.download_view_map(0, 0),
    "lfi_keep_views": lambda ctx: ctx.keep_views(0, 1),
    "lfi_compare_views": lambda ctx: ctx.compare_views(np.zeros((1, ctx.height, ctx.width, 4), np.uint8)),
    "lfi_download_quilt_tiles": lambda ctx: ctx.download_quilt_tiles(np.zeros((ctx.height, ctx.width, 4), np.uint8), 1, 1, 0, 1),
    "lfi_download_quilt_scaled": lambda ctx: ctx.download_quilt_scaled(1, 1, 8, 8),
    "lfi_download_views_yuv420": lambda ctx: ctx.download_views_yuv420(0, 1),
    "lfi_render_stream": lambda ctx: ctx.render_stream("STD", np.zeros((1, ctx.n_images), np.uint16)),
    "lfi_attach_views": lambda ctx: ctx.attach_views(256, 1 << 30),
    "lfi_release_inputs": lambda ctx: ctx.release_inputs(),
    "lfi_debug_derived_layout": lambda ctx: ctx.derived_layout(),
}


def bare_refusals(ctx):
    """{call: message} of BARE on a context without parameters; a call that is served is an assertion"""
    out, before = {}, memory(ctx)
    for name, call in BARE.items():
        try:
            call(ctx)
        except L.LfiError as e:
            out[name] = str(e)
        else:
            raise AssertionError(f"{name} was served on a context without parameters")
    assert memory(ctx) == before, ("a refused call changed lfi_memory_info", before, memory(ctx))
    return out


# ---- changes ------------------------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Change:
    name: str
    family: str
    before: State
    after: State
    again: str = None          # "grid" / "params": the call is made although its arguments are the before-state's
    sizes: tuple = ()          # (size, "grows" / "shrinks"): the ONE size of N, W, H, V, held rows that changes, where only one does


def _c(name, family, before, after, **kw):
    return Change(name, family, before, after, **kw)


def _both(name, family, a, b, size=None):
    grow = ((size, "grows"),) if size else ()
    shrink = ((size, "shrinks"),) if size else ()
    return [_c(f"{name}_up", family, a, b, sizes=grow), _c(f"{name}_down", family, b, a, sizes=shrink)]


OTHER = 0x2E2E                                   # other images: a change that keeps every size must not keep the answer
BAND = replace(TALL, window=(10, 18))            # interior: held rows (9, 19)
BAND_LARGER = replace(TALL, window=(8, 24))      # held rows (7, 25)
BAND_ELSEWHERE = replace(TALL, window=(22, 30))  # as many rows as BAND, other rows: every kept buffer has the right size and the wrong rows
SMALL_P = replace(SMALL, layout="planar")
FAR = replace(SMALL, focus=iw.FOCUS_LARGE)
FAR_P = replace(FAR, layout="planar")            # the three view flags want the planar layout, and offsets that leave the frame
LINEAR_P = replace(FAR_P, flags=LINEAR)
VIEW_MAPS = replace(SMALL, rows_kind="view_maps")
VARIANT = replace(SMALL, variant=OTHER_KERNELS)

CHANGES = (
    # lfi_set_grid
    _both("grid_small_large", "set_grid", SMALL, LARGE)
    + _both("grid_width", "set_grid", SMALL, replace(SMALL, W=300), "W")
    + _both("grid_height", "set_grid", SMALL, TALL, "H")
    + _both("grid_images", "set_grid", SMALL, replace(SMALL, cols=9, rows=8), "N")
    + [_c("grid_rearranged_4x4_2x8", "set_grid", replace(SMALL, cols=4, rows=4), replace(SMALL, cols=2, rows=8, seed=OTHER)),
       _c("grid_same_dimensions_again", "set_grid", SMALL, replace(SMALL, seed=OTHER), again="grid")]
    # lfi_set_row_window
    + [_c("window_none_to_band", "set_row_window", TALL, BAND, sizes=(("held", "shrinks"),)),
       _c("window_band_to_larger", "set_row_window", BAND, BAND_LARGER, sizes=(("held", "grows"),)),
       _c("window_larger_to_band", "set_row_window", BAND_LARGER, BAND, sizes=(("held", "shrinks"),)),
       _c("window_band_moved", "set_row_window", BAND, BAND_ELSEWHERE),
       _c("window_band_to_whole_image", "set_row_window", BAND, replace(TALL, window=(0, TALL.H)), sizes=(("held", "grows"),)),
       _c("window_band_then_set_grid", "set_row_window", BAND, replace(TALL, seed=OTHER), again="grid")]
    # lfi_set_params
    + _both("params_views_5_7", "set_params", SMALL, replace(SMALL, V=7), "V")        # the same v_pad: an equal blob total, another view count
    + _both("params_views_5_70", "set_params", SMALL, replace(SMALL, V=70), "V")
    + _both("params_focus_ids_9_4", "set_params", SMALL, replace(SMALL, ids=4))
    + _both("params_block_radius", "set_params", SMALL, replace(SMALL, radius=(4, 2)))
    + _both("params_focus_far", "set_params", SMALL, FAR)                                # planar_reach and pad_shift grow, then are larger than needed
    + _both("params_flag_deep", "set_params", FAR_P, replace(FAR_P, flags=DEEP))
    + _both("params_flag_in_frame", "set_params", FAR_P, replace(FAR_P, flags=IN_FRAME))
    + _both("params_flag_linear", "set_params", FAR_P, LINEAR_P)
    # from one flagged kernel to another: linear <-> deep (the deep views go, the planes stay allocated with the views: _check_memory) and
    # linear <-> in-frame; then the flag kept across another view count and across lfi_set_grid
    + _both("params_flag_linear_deep", "set_params", LINEAR_P, replace(FAR_P, flags=DEEP))
    + _both("params_flag_linear_in_frame", "set_params", LINEAR_P, replace(FAR_P, flags=IN_FRAME))
    + [_c("linear_then_more_views", "set_params", LINEAR_P, replace(LINEAR_P, V=70), sizes=(("V", "grows"),)),
       _c("linear_then_set_grid", "set_grid", LINEAR_P, replace(LINEAR_P, W=300), sizes=(("W", "grows"),))]
    + _both("params_flag_per_batch", "set_params", SMALL, replace(SMALL, flags=PER_BATCH))
    + _both("params_weights_wide", "set_params", SMALL, replace(SMALL, wide=True))       # weights_scalable
    # lfi_set_output_layout
    + _both("layout_rgba_planar", "set_output_layout", SMALL, SMALL_P)
    # lfi_attach_views: a caller's buffer sized for the after-state; then fewer views, which it still holds, and more, which it does not
    + [_c("attach_views", "attach_views", SMALL, replace(SMALL, V=7, views=7)),
       _c("attach_views_then_fewer_views", "attach_views", replace(SMALL, V=7, views=7), replace(SMALL, V=5, views=7), sizes=(("V", "shrinks"),)),
       _c("attach_views_then_more_views", "attach_views", replace(SMALL, V=5, views=7), replace(SMALL, V=70), sizes=(("V", "grows"),))]
    # lfi_attach_grid
    + [_c("attach_grid", "attach_grid", SMALL, replace(SMALL, inputs="attached", seed=OTHER)),
       _c("attach_grid_then_set_grid", "attach_grid", replace(SMALL, inputs="attached", seed=OTHER), SMALL, again="grid")]
    # lfi_release_inputs
    + [_c("release_inputs", "release_inputs", SMALL, replace(SMALL, inputs="released")),
       _c("release_then_set_grid_other_size", "release_inputs", replace(SMALL, inputs="released"), replace(LARGE, V=5)),
       _c("release_then_row_window_and_upload", "release_inputs", replace(TALL, inputs="released"), replace(BAND, seed=OTHER))]
    # context settings
    + [_c("focus_steps_32_256", "set_focus_steps", SMALL, replace(SMALL, steps=256)),
       _c("focus_steps_256_64", "set_focus_steps", replace(SMALL, steps=256), replace(SMALL, steps=64))]
    + _both("yuv_out_siting_left", "set_yuv_siting", SMALL, replace(SMALL, siting=("centre", "left")))
    + _both("yuv_in_siting_left", "set_yuv_siting", SMALL, replace(SMALL, siting=("left", "centre")))
    + _both("stream_callers", "set_stream", SMALL, replace(SMALL, stream="caller"))
    # lfi_set_variant for STD and TEN_WM: a setting that the later calls must leave alone (the kernel's name is asserted)
    + _both("variant_other_kernels", "set_variant", SMALL, VARIANT)
    + [_c("variant_then_params_other_views", "set_variant", VARIANT, replace(VARIANT, V=7), sizes=(("V", "grows"),)),
       _c("variant_then_set_grid", "set_variant", VARIANT, replace(VARIANT, W=300), sizes=(("W", "grows"),)),
       _c("variant_then_row_window", "set_variant", replace(TALL, variant=OTHER_KERNELS), replace(BAND, variant=OTHER_KERNELS), sizes=(("held", "shrinks"),))]
    # per-view rows
    + [_c("rows_int_set", "view_rows", SMALL, replace(SMALL, rows_kind="int")),
       _c("rows_float_set", "view_rows", SMALL, replace(SMALL, rows_kind="float")),
       _c("rows_view_maps_set", "view_rows", SMALL, VIEW_MAPS),
       _c("rows_int_then_params_same_views", "view_rows", replace(SMALL, rows_kind="int"), SMALL, again="params"),           # rows cleared, buffers kept
       _c("rows_view_maps_then_params_same_views", "view_rows", VIEW_MAPS, SMALL, again="params"),
       _c("rows_view_maps_then_more_views", "view_rows", VIEW_MAPS, replace(VIEW_MAPS, V=70), sizes=(("V", "grows"),)),      # the v_pad pitch changes
       _c("rows_view_maps_then_fewer_views", "view_rows", replace(VIEW_MAPS, V=70), VIEW_MAPS, sizes=(("V", "shrinks"),)),
       _c("rows_view_maps_then_set_grid", "view_rows", VIEW_MAPS, replace(SMALL, W=300, rows_kind="float"))]
)
assert len({c.name for c in CHANGES}) == len(CHANGES)
FAMILIES = ("set_grid", "set_row_window", "set_params", "set_output_layout", "attach_views", "attach_grid", "release_inputs", "set_focus_steps",
            "set_yuv_siting", "set_stream", "set_variant", "view_rows")
# changes after which no probe's expected output differs, by what they are: the issue they guard is a lost wait or a lost buffer, which shows
# as a wrong answer, not as the previous one
NO_OUTPUT_CHANGES = {"layout_rgba_planar_up": "the downloads are layout-independent; render_stream flips between served and refused",
                     "layout_rgba_planar_down": "as above", "release_inputs": "the same inputs from the planar copy alone; the focus readers flip to refused",
                     "stream_callers_up": "a stream changes no output", "stream_callers_down": "a stream changes no output",
                     "variant_other_kernels_up": "another kernel, the same bytes: the kernel's name is what std and ten_wm assert",
                     "variant_other_kernels_down": "as above",
                     "params_flag_deep_up": "the 8-bit bytes are the flag-free bytes; the deep codes exist under the flag alone (deep_views flips)",
                     "params_flag_deep_down": "as above",
                     "params_flag_per_batch_up": "the expected bytes are M16 either way: the per-batch mode must equal them, the default route stay within one LSB",
                     "params_flag_per_batch_down": "as above"}

# the functions of include/lfi.h that CHANGES stands for
CHANGE_CALLS = {"lfi_set_grid", "lfi_set_row_window", "lfi_set_params", "lfi_set_output_layout", "lfi_attach_views", "lfi_attach_grid", "lfi_grid_modified",
                "lfi_release_inputs", "lfi_set_focus_steps", "lfi_set_yuv_siting", "lfi_set_stream", "lfi_set_view_offsets", "lfi_set_view_float_offsets",
                "lfi_view_focus_maps", "lfi_set_variant"}
# … that are a step of a change and also what a probe calls, on purpose (lfi_set_variant: the FOCUS variants, and the readers of
# input_writers, which set "auto" for themselves)
CHANGE_AND_PROBE = {"lfi_set_view_offsets", "lfi_set_view_float_offsets", "lfi_view_focus_maps", "lfi_set_variant"}

EXCLUDED = {
    "lfi_create": "the frame of every case: each opens its contexts with it",
    "lfi_destroy": "the frame of every case; the long-lived test ends with it and a fresh context",
    "lfi_last_error": "reads the message of the last failure: every refusal here is matched through it",
    "lfi_abi_version": "a constant of the library, no context",
    "lfi_device_count": "asks the runtime, takes no context",
    "lfi_memory_info": "the measure of the memory checks and of every refusal, not a subject",
    "lfi_upload_wait": "a wait; changes and reads nothing",
    "lfi_broadcast_grid": "needs two devices (tests/test_distributed.py)",
    "lfi_view_layout": "reads width, rows and layout only; move sizes the attached view buffer by it, so a wrong answer fails lfi_attach_views",
    "lfi_views_device_ptr": "a pointer and a size; no buffer is read through it here",
    "lfi_focus_steps": "the getter of lfi_set_focus_steps: one integer",
    "lfi_yuv_siting": "the getter of lfi_set_yuv_siting: two integers",
    "lfi_focus_tiles_steps": "lfi_focus_tiles with another number of candidates: the same buffers (curve_ws, focus_ws), probed at 32",
    "lfi_focus_tiles_passes": "reads one integer of the last lfi_focus_tiles call",
    "lfi_focus_route_info": "reads the record of the last estimate call and its counts on the device; writes nothing",
    "lfi_std_band_info": "a per-device measurement, no context state",
    "lfi_benchmark": "renders in a loop; what it leaves is what lfi_render leaves",
    "lfi_timer_start": "records an event; reads and changes no buffer",
    "lfi_timer_stop": "records an event and waits; reads and changes no buffer",
    "lfi_download_quilt": "lfi_download_quilt_tiles over every tile: probed in two parts",
    "lfi_download_quilt_tiles_scaled": "lfi_download_quilt_scaled is this call over every tile: probed whole",
    "lfi_render_stream_yuv420": "lfi_render_stream's loop with lfi_download_views_yuv420's conversion per block, both probed; it allocates `yuv[2]` as they do",
    "lfi_yuv_surfaces_check": "pure: no context",
    "lfi_yuv_surfaces_packed": "pure: no context",
    "lfi_mosaic_map": "pure: no context",
    "lfi_debug_mosaic_chunk": "pure: no context",
    "lfi_debug_set_mosaic_chunk_cap": "a test knob of the mosaic uploads (input_writers.WRITERS owns them)",
    "lfi_upload_view_map": "writes a view's focus maps; state_rows reads the maps lfi_view_focus_maps estimated",
    "lfi_compare_view": "lfi_compare_views for one view: the same code (tests/test_gpu_compare_views.py holds them byte for byte)",
    "lfi_alloc_pinned": "host memory, no context",
    "lfi_free_pinned": "host memory, no context",
    "lfi_list_variants": "a constant list",
    "lfi_download_coords": "a debug dump with a local buffer",
    "lfi_download_prequant": "a debug dump; `prequant` is grow, one size per grid, released by free_grid - no probe yet",
    "lfi_debug_mfma_f16": "an instruction probe, no context state",
    "lfi_debug_mfma_f16_chain": "an instruction probe, no context state",
    "lfi_debug_pk_minmax3_f16": "an instruction probe, no context state",
    "lfi_debug_streams": "the stream handles: tests/stream_order.py",
}


def classify(name):
    """'change' / 'probe' / 'writer' / 'excluded' / None for a function of include/lfi.h; a change that input_writers also names is a change"""
    if name in CHANGE_CALLS:
        return "change"
    if any(name in p.calls for p in PROBES):
        return "probe"
    if name in {f for w in iw.WRITERS for f in w.abi}:
        return "writer"
    if name in EXCLUDED:
        return "excluded"
    return None


# ---- the discrimination check (CPU, oracle and restatements alone) ------------------------------------------------------------------------------------

def discrimination(oc, change):
    """For every probe that runs in both states of the change: (probe name, verdict, figure).  verdict "differs": the expected outputs have one
    shape and differ — a colour probe's in the given fraction of the compared bytes; "shape": they have different shapes (a stale answer
    cannot even be downloaded); "independent": the probe's output depends on fields of the state none of which changes (Probe.fields) — it
    is dropped from this change, and its two expected outputs must then BE equal; "flips": the probe runs in one state only."""
    out = []
    for p in PROBES:
        a, b = p.mode(change.before), p.mode(change.after)
        if p.name == "download_derived":
            continue          # its expected bytes follow the layout the context reports
        if (a == RUN) != (b == RUN):
            out.append((p.name, "flips", 0.0))
            # a probe that exists in one state only, against the probe whose answer a context that ignored the change would give there
            here, there = (change.before, change.after) if a == RUN else (change.after, change.before)
            q = next((q for q in PROBES if hasattr(p, "counterpart") and q.name == p.counterpart(here)), None)
            if q is not None and q.mode(there) == RUN:
                x, y = p.compared(p.want(oc, here), here), q.compared(q.want(oc, there), there)
                out.append((f"{p.name} against {q.name}", "shape" if x.shape != y.shape else "differs", 1.0 if x.shape != y.shape else float((x != y).mean())))
        if a != RUN or b != RUN:
            continue
        x, y = p.compared(p.want(oc, change.before), change.before), p.compared(p.want(oc, change.after), change.after)
        if p.depends(change.before) == p.depends(change.after):
            assert x.shape == y.shape and (x == y).all(), (change.name, p.name, "declared independent of the change, and its expected output changes")
            out.append((p.name, "independent", 0.0))
        elif x.shape != y.shape:
            out.append((p.name, "shape", 1.0))
        else:
            out.append((p.name, "differs", float((x != y).mean())))
    return out


def dropped(change):
    """[(probe name, reason)]: the probes that run in both states of the change and are dropped from it because their expected output cannot
    tell the two apart — by their declared fields, none of which the change touches; discrimination() holds each to equal outputs"""
    out = []
    for p in PROBES:
        if p.mode(change.before) == RUN and p.mode(change.after) == RUN and p.name != "download_derived" and p.depends(change.before) == p.depends(change.after):
            out.append((p.name, "its expected output depends on " + ", ".join(p.fields) + " alone, and the change touches none of them"))
    return out


# (change name, probe name) -> reason: every pair dropped from the table
DROPPED = {(c.name, name): reason for c in CHANGES for name, reason in dropped(c)}


# ---- the walk of the long-lived context ----------------------------------------------------------------------------------------------------------

def _plain(st, **kw):
    """the state with the fields that a window, a release or a flag cannot go with set back"""
    return replace(st, **{**dict(window=None, inputs="owned", flags=0, wide=False, rows_kind=None, views=0), **kw})


# (family, name, state -> state or None where the step does not apply, again)
STEPS = [
    ("set_grid", "to_large", lambda s: _plain(s, cols=9, rows=8, W=300, H=40, V=min(s.V, 7), focus=0.05) if s.dims != LARGE.dims and s.variant == AUTO else None, None),
    ("set_grid", "to_small", lambda s: _plain(s, cols=3, rows=3, W=136, H=24, focus=0.05) if s.dims != SMALL.dims else None, None),
    ("set_grid", "to_tall", lambda s: _plain(s, cols=3, rows=3, W=136, H=40, focus=0.05) if s.dims != TALL.dims else None, None),
    ("set_grid", "wider", lambda s: _plain(s, W=300, focus=0.05) if s.W == 136 else None, None),
    ("set_grid", "narrower", lambda s: _plain(s, W=136, focus=0.05) if s.W == 300 else None, None),
    ("set_grid", "more_images", lambda s: _plain(s, cols=9, rows=8, focus=0.05) if s.n == 9 and s.variant == AUTO else None, None),
    ("set_grid", "fewer_images", lambda s: _plain(s, cols=3, rows=3, focus=0.05) if s.n == 72 else None, None),
    ("set_grid", "same_again", lambda s: _plain(s, seed=s.seed ^ 0x3131), "grid"),
    ("set_row_window", "band", lambda s: _plain(s, window=(10, 18), focus=0.05, layout=s.layout) if s.H == 40 and not s.windowed else None, None),
    ("set_row_window", "band_larger", lambda s: replace(s, window=(8, 24)) if s.windowed and s.window != (8, 24) else None, None),
    ("set_row_window", "band_moved", lambda s: replace(s, window=(22, 30)) if s.windowed and s.window != (22, 30) else None, None),
    ("set_row_window", "whole", lambda s: replace(s, window=(0, s.H)) if s.windowed else None, None),
    ("set_params", "views_7", lambda s: replace(s, V=7, views=0) if s.V != 7 and not s.views else None, None),
    ("set_params", "views_5", lambda s: replace(s, V=5) if s.V != 5 else None, None),
    ("set_params", "views_70", lambda s: replace(s, V=70, views=0) if s.V != 70 and s.n == 9 and not s.windowed else None, None),
    ("set_params", "ids", lambda s: replace(s, ids=4 if s.ids == 9 else 9), None),
    ("set_params", "radius", lambda s: replace(s, radius=None if s.radius else (4, 2)), None),
    ("set_params", "focus", lambda s: replace(s, focus=iw.FOCUS_LARGE if s.focus == 0.05 else 0.05) if not s.windowed and s.inputs != "released" else None, None),
    ("set_params", "deep", lambda s: replace(s, flags=DEEP, wide=False, rows_kind=None) if s.layout == "planar" and not s.windowed and not s.flags and s.variant == AUTO else None, None),
    ("set_params", "in_frame", lambda s: replace(s, flags=IN_FRAME, wide=False, rows_kind=None) if s.layout == "planar" and not s.windowed and not s.flags and s.variant == AUTO else None, None),
    ("set_params", "linear", lambda s: replace(s, flags=LINEAR, wide=False, rows_kind=None) if s.layout == "planar" and not s.windowed and not s.flags and s.variant == AUTO else None, None),
    ("set_params", "per_batch", lambda s: replace(s, flags=PER_BATCH, rows_kind=None) if not s.windowed and not s.flags and s.inputs != "released" and s.variant == AUTO else None, None),
    ("set_params", "no_flags", lambda s: replace(s, flags=0) if s.flags else None, None),
    ("set_params", "weights", lambda s: replace(s, wide=not s.wide) if not s.windowed and not s.flags & VIEW_FLAGS and s.inputs != "released" and s.variant == AUTO else None, None),
    ("set_output_layout", "layout", lambda s: replace(s, layout="planar" if s.layout == "rgba" else "rgba", views=0) if not s.flags & VIEW_FLAGS else None, None),
    ("attach_views", "attach", lambda s: replace(s, views=max(s.V, 7)) if not s.views else None, None),
    ("attach_grid", "attach", lambda s: replace(s, inputs="attached", seed=s.seed ^ 0x3131) if s.inputs == "owned" else None, None),
    ("attach_grid", "back_to_owned", lambda s: _plain(s, layout=s.layout) if s.inputs == "attached" else None, "grid"),
    ("release_inputs", "release", lambda s: replace(s, inputs="released") if s.inputs == "owned" and not s.rows_kind and not s.windowed and not s.wide and not s.flags & PER_BATCH and s.variant == AUTO else None, None),
    ("set_focus_steps", "steps", lambda s: replace(s, steps={32: 256, 256: 64, 64: 32}[s.steps]), None),
    ("set_yuv_siting", "siting", lambda s: replace(s, siting=("centre", "left" if s.siting[1] == "centre" else "centre")), None),
    ("set_stream", "stream", lambda s: replace(s, stream="caller" if s.stream == "own" else "own"), None),
    ("set_variant", "other_kernels", lambda s: replace(s, variant=OTHER_KERNELS) if s.variant == AUTO and s.n == 9 and s.inputs != "released" and not s.flags and not s.wide and not s.rows_kind else None, None),
    ("set_variant", "auto", lambda s: replace(s, variant=AUTO) if s.variant != AUTO else None, None),
    ("view_rows", "int", lambda s: replace(s, rows_kind="int") if _rows_ok(s) and s.rows_kind != "int" else None, None),
    ("view_rows", "view_maps", lambda s: replace(s, rows_kind="view_maps") if _rows_ok(s) and s.rows_kind != "view_maps" and s.V <= 7 else None, None),
    ("view_rows", "cleared", lambda s: replace(s, rows_kind=None) if s.rows_kind else None, None),
]


def _rows_ok(s):
    return not s.windowed and s.inputs == "owned" and not s.flags and s.variant == AUTO


def walk(n=40, seed=20992):
    """[(family, name, after-state, again)]: a seeded walk from SMALL; a drawn step that does not apply in the current state gives way to the
    next drawn one.  tests/test_context_reuse_table.py holds the walk to every family and to both directions of N, W, H, V and the held rows."""
    rng = np.random.default_rng(seed)
    st, out = SMALL, []
    while len(out) < n:
        for i in rng.permutation(len(STEPS)):
            family, name, fn, again = STEPS[int(i)]
            after = fn(st)
            if after is None or (after == st and not again):
                continue
            out.append((family, name, after, again))
            st = after
            break
    return out
