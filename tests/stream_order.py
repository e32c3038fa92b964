"""Asynchronous calls held to stream order: a stalled-stream harness and the table of scripts it runs.

A context works on three streams — the compute stream (its own or a caller's), the copy stream and the side stream of the focus estimate —
and orders them with events.  include/lfi.h promises on top of them that calls are enqueued "without a host wait", that "renders already
enqueued keep the parameters they were enqueued with" and that "the context's stream is not drained".  A test that issues two calls and
compares bytes sees a missing wait only while the GPU is still busy with the first call, which at the suite's shapes it never is.

Here the race window is opened on purpose.  A finite spin (torch.cuda._sleep) is put on ONE of the streams, a whole script of calls is issued
behind it from the host, and only then does the GPU catch up.  Work on another stream that fails to wait for the stalled one runs during
the stall and leaves wrong bytes every time; the same run shows that no call blocked the host (the stall's end event is still pending when
the last asynchronous call has returned).  Every script runs with the stall on the compute stream, on the copy stream and on the side stream.

A script is a function of a recorder (Rec).  Run dry (no context) it carries the state of the context on the host — the grid, the
parameters, the maps, what the views hold — and records what every snapshot must show as a State; the oracle turns a State into bytes.  Run
live it issues the same steps on a context.  Nothing the harness expects comes from the library.

This file imports without a GPU: tests/test_stream_order_table.py (CPU) holds CLASSES to the header and every script to being a check,
tests/test_gpu_stream_order.py runs script x placement.
"""
import os
import sys
import time
from dataclasses import dataclass, replace

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:          # as tests/conftest.py does: this file is also run as a program (main, below)
    sys.path.insert(0, _ROOT)

import input_writers as iw
import mosaic_ref as mref
import ten_interval
import yuv_ref
import yuv_surfaces_ref as sref

TRAJ, EFFECT, ASPECT = "0.071,0.071,0.93,0.93", 3.0, 1.783
W, H, V = 200, 24, 8
PLACEMENTS = ("compute", "copy", "aux")
STALL_FACTOR, STALL_MIN_MS, STALL_MAX_MS = 5.0, 50.0, 500.0
CANARY_MS = 20.0          # the other streams' events complete within this while the stall is pending, or the streams share a hardware queue
TEN_TOL_LSB = 1
POISON = (0xA5, 0x5A)

# ---- every function of include/lfi.h, by what it may do to the calling thread ------------------------------------------------------------------
# ASYNC: enqueues and returns; must not wait for the device.  COND: asynchronous except under the quoted condition.  SYNC: documented to
# wait (or to return results, which is the same).  HOST: no device work at all.
ASYNC, COND, SYNC, HOST = "asynchronous", "conditionally blocking", "synchronous", "host-only"
RING = "two-slot staging ring: the third call in a row waits for the copy of the first"
CLASSES = {
    "lfi_create": (SYNC, "creates the stream and events"),
    "lfi_destroy": (SYNC, "drains the three streams"),
    "lfi_last_error": (HOST, ""), "lfi_abi_version": (HOST, ""), "lfi_device_count": (HOST, ""),
    "lfi_set_grid": (SYNC, "drains the stream, reallocates"),
    "lfi_set_row_window": (SYNC, "drains the stream, reallocates"),
    "lfi_upload_image": (SYNC, "\"Synchronous.\""),
    "lfi_upload_image_async": (ASYNC, "\"the call returns at once\" for a page-locked source"),
    "lfi_upload_wait": (SYNC, "\"host wait for the asynchronous uploads issued so far\""),
    "lfi_upload_images_yuv420": (COND, "waits for the copy stream when its device staging buffer has to grow (first use, more frames)"),
    "lfi_upload_images_yuv": (COND, "host or unaligned device surfaces: as lfi_upload_images_yuv420; device surfaces read in place never wait"),
    "lfi_upload_images_yuv_derived": (COND, "as lfi_upload_images_yuv"),
    "lfi_upload_mosaic_yuv": (COND, "as lfi_upload_images_yuv"),
    "lfi_upload_mosaic_yuv_derived": (COND, "as lfi_upload_images_yuv"),
    "lfi_upload_mosaic": (ASYNC, "\"lfi_upload_image_async of every tile's rectangle\""),
    "lfi_attach_grid": (SYNC, "waits for uploads and the stream"),
    "lfi_broadcast_grid": (SYNC, "\"Synchronous.\""),
    "lfi_release_inputs": (SYNC, "builds the copy, frees the planes"),
    "lfi_grid_device_ptr": (HOST, ""),
    "lfi_grid_modified": (HOST, "bookkeeping only: the write it announces is the caller's, in the caller's stream order"),
    "lfi_fill_synthetic": (ASYNC, ""), "lfi_fill_synthetic_images": (ASYNC, ""), "lfi_fill_synthetic_scene": (ASYNC, ""),
    "lfi_set_params": (COND, "\"A call that changes the number of views synchronises and reallocates\"; in place: " + RING),
    "lfi_set_view_offsets": (COND, "the first rows of a view count allocate behind a drained stream; then " + RING),
    "lfi_set_view_float_offsets": (COND, "as lfi_set_view_offsets"),
    "lfi_view_focus_maps": (COND, "the first call of a size allocates behind a drained stream; then " + RING),
    "lfi_set_output_layout": (SYNC, "frees the views"),
    "lfi_view_layout": (HOST, ""),
    "lfi_attach_views": (SYNC, "drains the stream, frees the views"),
    "lfi_views_device_ptr": (HOST, "allocates the views if there are none"),
    "lfi_focus_map": (COND, "the first call of a size allocates its workspace"),
    "lfi_set_focus_steps": (HOST, ""), "lfi_focus_steps": (HOST, ""),
    "lfi_focus_curve": (SYNC, "\"synchronous\""), "lfi_focus_tiles": (SYNC, "\"synchronous\""), "lfi_focus_tiles_steps": (SYNC, "\"synchronous\""),
    "lfi_focus_tiles_passes": (HOST, ""),
    "lfi_focus_route_info": (SYNC, "\"synchronises the context's streams and copies 64 bytes\" where the factored estimate ran"),
    "lfi_render": (COND, "the first STD launch over more than 64 images on a device runs the band's self-check (lfi_std_band_info); a planar "
                         "copy that has to grow is reallocated behind a drained stream"),
    "lfi_render_stream": (SYNC, "\"Returns after everything has completed.\""),
    "lfi_render_stream_yuv420": (SYNC, "as lfi_render_stream"),
    "lfi_prepare": (SYNC, "\"Optional; synchronous.\""),
    "lfi_memory_info": (HOST, ""),
    "lfi_std_band_info": (SYNC, "runs the check if it has not run"),
    "lfi_last_kernel_name": (HOST, ""),
    "lfi_benchmark": (SYNC, "\"Synchronous.\""),
    "lfi_timer_start": (ASYNC, "an event record"),
    "lfi_timer_stop": (SYNC, "\"records, synchronises\""),
    "lfi_sync": (SYNC, ""),
    "lfi_download_view": (SYNC, ""), "lfi_download_map": (SYNC, ""), "lfi_download_quilt": (SYNC, ""), "lfi_download_quilt_tiles": (SYNC, ""),
    "lfi_download_quilt_scaled": (SYNC, ""), "lfi_download_quilt_tiles_scaled": (SYNC, ""), "lfi_download_native": (SYNC, ""),
    "lfi_download_views_yuv420": (SYNC, ""), "lfi_download_views_yuv": (SYNC, ""), "lfi_download_quilt_yuv": (SYNC, ""),
    "lfi_download_rgbd_yuv": (SYNC, ""),
    "lfi_yuv_surfaces_check": (HOST, ""), "lfi_yuv_surfaces_packed": (HOST, ""), "lfi_set_yuv_siting": (HOST, ""), "lfi_yuv_siting": (HOST, ""),
    "lfi_mosaic_map": (HOST, ""), "lfi_debug_mosaic_chunk": (HOST, ""), "lfi_debug_set_mosaic_chunk_cap": (HOST, ""),
    "lfi_upload_map": (SYNC, ""), "lfi_download_view_map": (SYNC, ""), "lfi_upload_view_map": (SYNC, ""),
    "lfi_compare_view": (SYNC, ""), "lfi_compare_views": (SYNC, "\"synchronous\""),
    "lfi_keep_views": (COND, "\"no host synchronisation (unless the set's size changes: the old allocation is freed)\""),
    "lfi_alloc_pinned": (HOST, "hipHostMalloc"), "lfi_free_pinned": (HOST, "hipHostFree"),
    "lfi_set_stream": (ASYNC, "\"no host synchronisation\""),
    "lfi_set_variant": (HOST, ""), "lfi_list_variants": (HOST, ""),
    "lfi_download_coords": (SYNC, ""), "lfi_download_prequant": (SYNC, ""),
    "lfi_debug_mfma_f16": (SYNC, ""), "lfi_debug_pk_minmax3_f16": (SYNC, ""), "lfi_debug_mfma_f16_chain": (SYNC, ""),
    "lfi_debug_poison": (ASYNC, "\"hipMemsetAsync on the context's stream, ordered like every other call\""),
    "lfi_debug_derived_layout": (HOST, ""), "lfi_debug_download_derived": (SYNC, ""),
    "lfi_debug_streams": (HOST, "creates the two side streams if they do not exist"),
}
MUST_BE_SCRIPTED = (ASYNC, COND)


# ---- what a snapshot shows -------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class State:
    """what the views hold after a render: the method, the inputs g, the parameters h, the per-view rows and the map it read"""
    method: str
    af: bool
    g: int
    h: int
    rows: object = None     # None / ("int", i) / ("float", i)
    mp: object = None       # None / ("ctx", g, h, k): plane k of lfi_focus_map at (g, h) / ("view", g, h, i, k): the per-view maps over float rows i


@dataclass(frozen=True)
class Geometry:
    cols: int
    rows: int
    layout: str = "rgba"

    @property
    def n(self):
        return self.cols * self.rows

    @property
    def shape(self):
        return iw.Shape(f"g{self.cols}x{self.rows}", self.cols, self.rows, W, H, 0, (4, 2))


G8, G8P, G9, G9P = Geometry(8, 8), Geometry(8, 8, "planar"), Geometry(9, 9), Geometry(9, 9, "planar")
# (focus, range) of the parameter sets a script may switch between; the last is the largest reach (the released scripts stay on it)
PARAMS = [(0.05, 0.17), (0.23, 0.1), (0.4, 0.2), (0.11, 0.25), (0.31, 0.12)]
PATH_VIEWS = 2 * V + 3                               # lfi_render_stream: three blocks, the last one partial
PATH_TRAJ, PATH_EFFECT = TRAJ, 1.0                     # … with wider weights: the same trajectory, so the same offsets, and no block looks like the parameters' views
RAMPS = [(0.05, 0.4), (0.4, 0.05), (0.2, 0.6)]       # integer rows: the focus ramps
CENTRES = [1.0, 0.6, 1.4]                            # float rows: every view's camera-centred offsets, scaled (the rows are the caller's to choose)


class Oracle:
    """State -> bytes, on the host, cached"""

    def __init__(self, L, oc, geo, grids):
        self.L, self.oc, self.geo, self.grids = L, oc, geo, grids
        self.hps = [L.build_params(geo.cols, geo.rows, W, H, TRAJ, f, r, EFFECT, ASPECT, V) for f, r in PARAMS]
        self._memo = {}

    def path(self, h):
        """the parameters of a longer camera path at parameter set h: the same offsets (one trajectory centre), PATH_VIEWS rows of weights"""
        f, r = PARAMS[h]
        p = self.L.build_params(self.geo.cols, self.geo.rows, W, H, PATH_TRAJ, f, r, PATH_EFFECT, ASPECT, PATH_VIEWS)
        assert np.array_equal(p.offsets, self.hps[h].offsets) and np.array_equal(p.focused_offsets, self.hps[h].focused_offsets)
        return p

    def int_rows(self, i):
        D = self.L.build_view_offsets(self.geo.cols, self.geo.rows, W, H, TRAJ, ASPECT, self.L.focus_ramp(RAMPS[i][0], RAMPS[i][1], V))
        return np.ascontiguousarray(D, np.int32)

    def float_rows(self, i):
        O, _ = self.L.build_view_centred_offsets(self.geo.cols, self.geo.rows, W, H, TRAJ, ASPECT, np.full(V, PARAMS[0][0], np.float32))
        return np.ascontiguousarray(O * np.float32(CENTRES[i]), np.float32)

    def view_ids(self):
        return np.ascontiguousarray(self.L.build_view_focus_ids(self.geo.cols, self.geo.rows, TRAJ, V), np.int32)

    def _cached(self, key, fn):
        if key not in self._memo:
            self._memo[key] = fn()
        return self._memo[key]

    def maps(self, g, h, offsets=None, ids=None, tag=None):
        hp = self.hps[h]

        def compute():
            m0 = self.oc.focus_estimate(self.grids[g], hp.offsets if offsets is None else offsets, hp.focus_map_ids if ids is None else ids,
                                        hp.focus, hp.range, hp.block_radius, threads=8)
            return m0, self.oc.focus_filter(m0, hp.block_radius, threads=8)
        return self._cached(("maps", g, h, tag), compute)

    def view_maps(self, g, h, i):
        O, ids = self.float_rows(i), self.view_ids()
        return [self.maps(g, h, np.ascontiguousarray(O[v]), np.ascontiguousarray(ids[v]), ("view", i, v)) for v in range(V)]

    def _plane(self, st, v):
        if st.mp[0] == "ctx":
            return self.maps(st.mp[1], st.mp[2])[st.mp[3]]
        return self.view_maps(st.mp[1], st.mp[2], st.mp[3])[v][st.mp[4]]

    def _blend(self, fn, st, **extra):
        grid, hp = self.grids[st.g], self.hps[st.h]
        if st.rows is None:
            kw = dict(all_focus=True, map_plane=self._plane(st, 0), focus=hp.focus, rng=hp.range) if st.af else {}
            return fn(grid, hp.focused_offsets, hp.offsets, hp.weights, threads=8, **kw, **extra)
        out = []
        for v in range(V):
            w = np.ascontiguousarray(hp.weights[v:v + 1])
            if st.rows[0] == "int":
                D = self.int_rows(st.rows[1])[v].copy()
                D[:, 0], D[:, 1] = np.clip(D[:, 0], -W, W), np.clip(D[:, 1], -H, H)
                out.append(fn(grid, np.ascontiguousarray(D), hp.offsets, w, **extra)[0])
            else:
                O = np.ascontiguousarray(self.float_rows(st.rows[1])[v])
                out.append(fn(grid, hp.focused_offsets, O, w, all_focus=True, map_plane=self._plane(st, v), focus=hp.focus, rng=hp.range, **extra)[0])
        return np.stack(out)

    def views(self, st):
        """STD: the bytes.  TEN_WM: (M16, lo, hi) — within one LSB of the half-accumulator model and inside the interval of the exact sum"""
        def compute():
            if st.method == "STD":
                return self._blend(self.oc.blend_std, st)
            m16 = self._blend(self.oc.blend_ten, st, model=self.oc.TEN_M16)
            S = self._blend(self.oc.blend_f64, st)
            lo, hi = ten_interval.interval(S, ten_interval.epsilon(self.hps[st.h].weights, self.geo.n))
            return m16, lo, hi
        return self._cached(("views", st), compute)

    def colour(self, st):
        want = self.views(st)
        return (want if st.method == "STD" else want[0])[..., :3]

    def distinct(self, a, b):
        """the fraction of colour bytes in which no render of state a could pass for one of state b"""
        x, y = self.colour(a).astype(np.int32), self.colour(b).astype(np.int32)
        tol = 0 if a.method == "STD" and b.method == "STD" else 2 * TEN_TOL_LSB
        return float((np.abs(x - y) > tol).mean())


def check_views(got, want, method, what):
    if method == "STD":
        assert (got == want).all(), (what, "STD bytes differ", int((got != want).sum()), "of", got.size)
        return
    m16, lo, hi = want
    d = int(np.abs(got.astype(int) - m16.astype(int)).max())
    assert d <= TEN_TOL_LSB, (what, "TEN_WM: LSB from M16", d, "bytes beyond", int((np.abs(got.astype(int) - m16.astype(int)) > TEN_TOL_LSB).sum()))
    out = ten_interval.outside(got, lo, hi)
    assert out == 0, (what, "TEN_WM: bytes outside the interval of the exact sum", out)


# ---- writers: input_writers' factories at this file's runs, issued through a recording context so that their buffers are staged before the stall ----

def _half(n):
    return [(n // 4, n // 4 + n // 2)]


def _whole(n):
    return [(0, n)]


def _mosaic_geometry(s):
    return (s.cols, s.rows, "grid", False, 0, s.n, 0)


def _make_mosaic_rgba(env):
    """the whole grid from one host RGBA image of cols x rows tiles, its row pitch beyond the tiles"""
    s = env.shape
    image = np.random.default_rng(env.seed).integers(0, 256, (s.rows * s.H, s.cols * s.W + 5, 4), dtype=np.uint8)
    image[..., 3] = 255
    tiles = mref.mosaic_map(s.cols, s.rows, 0, s.n, mref.ROWS, 0, s.cols, s.rows, 0)
    return {"images": mref.rgba_tiles(image, s.W, s.H, tiles), "image": image}


def _apply_mosaic_rgba(L, ctx, p, env, keep):
    ctx.upload_mosaic(L.Mosaic.make(env.shape.cols, env.shape.rows, "rows"), p["image"], 0)


def _w(name, abi, runs, make_apply, released=False):
    return iw.Writer(name, abi, runs, make_apply[0], make_apply[1], released=released)


WRITERS = {w.name: w for w in [
    _w("upload_image_async", ("lfi_upload_image_async",), _half, iw._rgba(_half, iw._upload_async_pinned)),
    _w("upload_images_yuv420", ("lfi_upload_images_yuv420",), _half, iw._yuv8(_half, sref.I420, sref.tight, sref.HOST, iw.C709, via420=True)),
    _w("upload_images_yuv_host", ("lfi_upload_images_yuv",), _half, iw._yuv8(_half, sref.NV12, sref.pitched, sref.HOST, iw.C601F)),
    _w("upload_images_yuv_device", ("lfi_upload_images_yuv",), _half, iw._yuv8(_half, sref.NV12, sref.pitched, sref.DEVICE, iw.C709)),
    _w("upload_mosaic_yuv_device", ("lfi_upload_mosaic_yuv",), None, iw._mosaic_yuv(_mosaic_geometry, sref.I420, sref.pitched, sref.DEVICE, iw.C709)),
    _w("upload_mosaic", ("lfi_upload_mosaic",), None, (_make_mosaic_rgba, _apply_mosaic_rgba)),
    _w("fill_synthetic", ("lfi_fill_synthetic",), None, (iw._make_synthetic(_whole), lambda L, ctx, p, env, keep: ctx.fill_synthetic(p["seed"]))),
    _w("fill_synthetic_images", ("lfi_fill_synthetic_images",), _half,
       (iw._make_synthetic(_half), lambda L, ctx, p, env, keep: ctx.fill_synthetic(p["seed"], *_half(env.shape.n)[0]))),
    _w("fill_synthetic_scene", ("lfi_fill_synthetic_scene",), None, (iw._make_scene, lambda L, ctx, p, env, keep: ctx.fill_synthetic_scene(p["seed"]))),
    _w("attached_grid_write", ("lfi_grid_modified",), None, (iw._make_whole, None)),
    _w("upload_images_yuv_derived", ("lfi_upload_images_yuv_derived",), _half,
       iw._yuv8(_half, sref.NV12, sref.pitched, sref.HOST, iw.C709, derived=True), released=True),
    _w("upload_mosaic_yuv_derived", ("lfi_upload_mosaic_yuv_derived",), None,
       iw._mosaic_yuv(_mosaic_geometry, sref.I420, sref.tight, sref.HOST, iw.C709, derived=True), released=True),
]}


class _Recording:
    """stands in for the context while a writer's apply runs before the stall: page-locked memory is real, every other call is recorded"""

    def __init__(self, ctx):
        self._ctx, self.calls = ctx, []

    def pinned_empty(self, *a, **kw):
        return self._ctx.pinned_empty(*a, **kw)

    def __getattr__(self, name):
        def record(*a, **kw):
            self.calls.append((name, a, kw))
        return record


def _stage(L, ctx, writer, payload, env, keep):
    """the writer's calls with every host array in page-locked memory and every device buffer in place: [(method name, args, kwargs)]"""
    rec = _Recording(ctx)
    writer.apply(L, rec, payload, env, keep)

    def pinned(a):
        if not isinstance(a, np.ndarray):
            return a
        p = ctx.pinned_empty(a.shape, a.dtype)     # a pageable hipMemcpyAsync may legitimately wait for the stream
        p[...] = a
        return p
    return [(name, tuple(pinned(a) for a in args), kw) for name, args, kw in rec.calls]


# ---- the recorder ----------------------------------------------------------------------------------------------------------------------------

class Rec:
    """A script's steps.  Dry (live None): the host shadow and the expectations.  Live: the same, and the calls on the context."""

    def __init__(self, L, oc, script, live=None):
        self.L, self.oc, self.script, self.live = L, oc, script, live
        geo = script.geo
        if live is None:
            self.grids = [iw.first_grid(oc, geo.shape)]
            self.oracle = Oracle(L, oc, geo, self.grids)
        else:                         # the dry run's oracle and grids: the expectations are computed once per script
            self.oracle = live.plan.oracle
            self.grids = self.oracle.grids
        self.g = self.h = 0
        self.last_param = len(PARAMS) - 1 if script.released else 0
        self.h = self.last_param
        self.views = None            # State of what the views hold
        self.map_state = None        # (g, h) of the last lfi_focus_map
        self.rows_int = self.rows_float = None
        self.view_maps_state = None  # (g, h, i) while all-focus renders read the per-view maps
        self.view_maps_made = None   # … of the last lfi_view_focus_maps: the maps stay in device memory of their own
        self.h_seen = {self.h}
        self.snapshots = []          # (label, State)
        self.writes = []             # (writer, payload, env)
        self.used = set()            # the functions of lfi.h the script calls inside the window
        self.calls = []              # live: (label, seconds, may_block)
        self.streamed = []           # (kind, method, h, live: the host array) of every lfi_render_stream / lfi_render_stream_yuv420
        self.compare = None          # (State now, State kept) of the last compare_views
        self.compared = None         # live: its result
        self.in_place_params = self.rows_staged = 0
        self.checked_not_drained = False

    # -- plumbing --
    def _call(self, abi, label, fn, may_block=None):
        self.used.update(abi if isinstance(abi, tuple) else (abi,))
        if self.live is None:
            return None
        if may_block and not self.checked_not_drained:
            self.live.check_not_drained(self)
        t = time.perf_counter()
        out = fn(self.live.ctx)
        self.calls.append((label, time.perf_counter() - t, may_block))
        return out

    # -- steps --
    def set_params(self, h):
        """in place: the view count stays"""
        self.in_place_params += 1
        mb = RING if self.in_place_params >= 3 else None
        self.h = h
        self.h_seen.add(h)
        self.rows_int = self.rows_float = self.view_maps_state = None
        self._call("lfi_set_params", f"set_params({PARAMS[h]})", lambda ctx: ctx.set_params(self.oracle.hps[h]), mb)

    def render(self, method, af=False):
        rows = mp = None
        if af:
            if self.rows_float is not None:
                rows = ("float", self.rows_float)
            k = 1 if method == "STD" else 0       # Standard::process reads map 1, Tensors::process map 0 (lfi.h, LFI_FLAG_UNIFIED_FOCUS_MAP)
            if rows and self.view_maps_state is not None:
                mp = ("view",) + self.view_maps_state + (k,)
            else:
                assert self.map_state is not None, "an all-focus render without a map"
                mp = ("ctx",) + self.map_state + (k,)
        elif self.rows_int is not None:
            rows = ("int", self.rows_int)
        self.views = State(method, af, self.g, self.h, rows, mp)
        self._call("lfi_render", f"render({method}, all_focus={af})", lambda ctx: ctx.render(method, all_focus=af))

    def snapshot(self, label):
        assert self.views is not None
        self.snapshots.append((label, self.views))
        if self.live is not None:
            self.live.snapshot(len(self.snapshots) - 1)

    def focus_map(self):
        self.map_state = (self.g, self.h)
        self._call("lfi_focus_map", "focus_map", lambda ctx: ctx.focus_map())

    def poison_views(self):
        """in stream order, between two renders: a memset that ran early would show in the snapshot before it"""
        self.views = None
        self._call("lfi_debug_poison", "poison(views)", lambda ctx: ctx.poison(self.L.LFI_POISON_VIEWS, POISON[0]))

    def timer_start(self):
        self._call("lfi_timer_start", "timer_start", lambda ctx: ctx.timer_start())

    def write(self, name):
        writer, i = WRITERS[name], len(self.writes)
        if self.live is None:
            env = iw.Env(self.L, self.oc, self.script.geo.shape, 0x51 + i, "centre", self.oracle.hps[self.h])
            payload = writer.make(env)
            self.grids.append(iw.shadow_apply(self.grids[self.g], payload, writer))
            self.writes.append((writer, payload, env, len(self.grids) - 1))
        else:
            self.writes.append(self.live.plan.writes[i])
        self.g = self.writes[i][3]
        self._call(writer.abi, f"write({name})", lambda ctx: self.live.write(i))

    def set_view_offsets(self, i):
        self.rows_staged += 1
        self.rows_int = i
        D = self.oracle.int_rows(i)
        self._call("lfi_set_view_offsets", f"set_view_offsets(ramp {RAMPS[i]})", lambda ctx: ctx.set_view_offsets(D), RING if self.rows_staged >= 3 else None)

    def set_view_float_offsets(self, i):
        self.rows_staged += 1
        self.rows_float, self.view_maps_state = i, None
        O = self.oracle.float_rows(i)
        self._call("lfi_set_view_float_offsets", f"set_view_float_offsets(x {CENTRES[i]})", lambda ctx: ctx.set_view_float_offsets(O),
                   RING if self.rows_staged >= 3 else None)

    def view_focus_maps(self):
        assert self.rows_float is not None
        self.view_maps_state = self.view_maps_made = (self.g, self.h, self.rows_float)
        ids = self.oracle.view_ids()
        self._call("lfi_view_focus_maps", "view_focus_maps", lambda ctx: ctx.view_focus_maps(ids))

    def set_stream(self, which):
        """which: "s1" / "s2" (the caller's) / None (the context's own)"""
        self._call("lfi_set_stream", f"set_stream({which})", lambda ctx: self.live.set_stream(which))

    def keep_views(self):
        self.kept = self.views
        self._call("lfi_keep_views", "keep_views", lambda ctx: ctx.keep_views())

    def compare_views(self):
        self.compare = (self.views, self.kept)
        self.compared = self._call("lfi_compare_views", "compare_views(None)", lambda ctx: ctx.compare_views(None),
                                   "\"synchronous; ordered after the work on the stream in use\"")

    def render_stream(self, method, yuv=False):
        """a camera path of PATH_VIEWS views in blocks of V behind whatever is enqueued: synchronous by contract — what is held is that its
        weight copies do not reach the parameter arrays before the renders enqueued earlier have read them"""
        path = self.oracle.path(self.h)
        i = len(self.streamed)
        self.views = None              # the last block's views, its weights in the arrays: the script ends here or sets parameters
        abi = "lfi_render_stream_yuv420" if yuv else "lfi_render_stream"
        out = self.live.stream_out[i] if self.live is not None else None
        self.streamed.append(("yuv" if yuv else "rgba", method, self.g, self.h, out))
        why = "\"Returns after everything has completed.\""
        if yuv:
            self._call(abi, f"render_stream_yuv420({method})", lambda ctx: ctx.render_stream_yuv420(method, path.weights, out=out, matrix=yuv_ref.FORMATS[0][0],
                                                                                                      range=yuv_ref.FORMATS[0][1]), why)
        else:
            self._call(abi, f"render_stream({method})", lambda ctx: ctx.render_stream(method, path.weights, out), why)

    # -- what the run must show --
    def streamed_want(self, i):
        """the oracle's views of the whole path (STD: bytes; TEN_WM: M16, lo, hi), as YUV frames where the call makes them (STD only)"""
        kind, method, g, h, _ = self.streamed[i]
        path, grid = self.oracle.path(h), self.grids[g]
        if method == "STD":
            views = self.oc.blend_std(grid, path.focused_offsets, path.offsets, path.weights, threads=8)
            return yuv_ref.frames(views, *yuv_ref.FORMATS[0]) if kind == "yuv" else views
        assert kind == "rgba"
        lo, hi = ten_interval.bounds(self.oc, grid, path, threads=8)
        return self.oc.blend_ten(grid, path.focused_offsets, path.offsets, path.weights, model=self.oc.TEN_M16, threads=8), lo, hi

    def final_maps(self):
        return None if self.map_state is None else self.oracle.maps(*self.map_state)

    def confusable(self):
        """for every snapshot: the states it must not be mistaken for — the same render from any other inputs, parameters, rows or map of
        this script, and what any other snapshot of the script shows (kept or not re-rendered views)"""
        gs, hs = range(len(self.grids)), sorted(self.h_seen)
        ctx_maps = sorted({s.mp[1:3] for _, s in self.snapshots if s.mp and s.mp[0] == "ctx"} | ({self.map_state} if self.map_state else set()))
        rows = sorted({s.rows for _, s in self.snapshots if s.rows}, key=repr)
        out = []
        for label, s in self.snapshots:
            alts = {replace(s, g=g) for g in gs} | {replace(s, h=h) for h in hs}
            if s.mp and s.mp[0] == "ctx":
                alts |= {replace(s, mp=("ctx",) + m + (k,)) for m in ctx_maps for k in (0, 1)}
            if s.mp and s.mp[0] == "view":
                alts |= {replace(s, mp=s.mp[:4] + (1 - s.mp[4],))}
                if self.map_state:
                    alts |= {replace(s, mp=("ctx",) + self.map_state + (k,)) for k in (0, 1)}
            if s.rows:
                alts |= {replace(s, rows=r) for r in rows if r[0] == s.rows[0]}
                if s.rows[0] == "int":
                    alts.add(replace(s, rows=None))
            alts |= {t for _, t in self.snapshots}
            alts = {t for t in alts if replace(t, method=s.method) != s}     # the two methods' renders of one state are meant to look alike
            out.append((label, s, sorted(alts, key=repr)))
        return out


# ---- scripts -----------------------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Script:
    name: str
    geo: Geometry
    body: object
    attached: bool = False     # the grid is a caller-owned tensor (lfi_attach_grid), announced once
    released: bool = False     # after lfi_release_inputs
    caller: bool = False       # starts on the caller's stream s1: "compute" stalls s1


def _params_war(method):
    def body(r):
        r.timer_start()
        r.render(method); r.snapshot("before: parameters 0")
        r.set_params(1)
        r.set_params(2)
        r.render(method); r.snapshot("after two in-place set_params: parameters 2")
    return body


def _params_four(method, renders):
    def body(r):
        r.render(method); r.snapshot("parameters 0")
        for i in (1, 2, 3, 4):
            r.set_params(i)
            if renders or i == 4:
                r.render(method); r.snapshot(f"parameters {i}")
    return body


def _focus_side_stream(r):
    r.focus_map()
    r.render("TEN_WM", af=True); r.snapshot("TEN_WM reads map 0 beside the filter")
    r.render("STD", af=True); r.snapshot("STD reads map 1: joins the filter")
    r.set_params(1)
    r.set_params(2)
    r.focus_map()
    r.render("TEN_WM", af=True); r.snapshot("TEN_WM, second map 0")
    r.render("STD", af=True); r.snapshot("STD, second map 1")


def _writer(name, methods=("TEN_WM", "STD")):
    def body(r):
        for m in methods:
            r.render(m); r.snapshot(f"{m} before the write")
        r.write(name)
        for m in methods:
            r.render(m); r.snapshot(f"{m} after the write")
    return body


def _writer_focus(name):
    """the estimate's padded planes are a derived copy too"""
    def body(r):
        r.focus_map()
        r.render("STD", af=True); r.snapshot("all-focus before the write")
        r.write(name)
        r.focus_map()
        r.render("STD", af=True); r.snapshot("all-focus after the write")
    return body


def _int_rows(r):
    for i in (0, 1, 2):
        r.set_view_offsets(i)
        r.poison_views()
        r.render("STD"); r.snapshot(f"integer rows {i}")


def _float_rows(r):
    r.focus_map()
    for i in (0, 1, 2):
        r.set_view_float_offsets(i)
        r.render("STD", af=True); r.snapshot(f"float rows {i}")


def _view_maps(r):
    r.focus_map()
    r.set_view_float_offsets(1)
    r.view_focus_maps()
    r.render("TEN_WM", af=True); r.snapshot("TEN_WM over per-view maps 0")
    r.render("STD", af=True); r.snapshot("STD over per-view maps 1")
    r.focus_map()
    r.set_params(2)
    r.focus_map()
    r.render("STD", af=True); r.snapshot("STD over the context's map again")


def _switch(r):
    r.render("STD"); r.snapshot("on s1")
    r.set_params(1)
    r.set_stream("s2")
    r.render("STD"); r.snapshot("on s2, parameters 1")
    r.set_params(2)
    r.set_stream(None)
    r.render("TEN_WM"); r.snapshot("back on the context's stream, parameters 2")


def _switch_filter(r):
    r.focus_map()
    r.set_stream("s2")
    r.render("STD", af=True); r.snapshot("map 1 from the filter pending on the side stream")
    r.set_stream(None)
    r.set_params(1)
    r.focus_map()
    r.render("TEN_WM", af=True); r.snapshot("second map 0")


def _switch_uploads(r):
    r.render("TEN_WM"); r.snapshot("on s1 before the upload")
    r.write("upload_image_async")
    r.set_stream("s2")
    r.render("TEN_WM"); r.snapshot("on s2 behind the uploads pending on the copy stream")
    r.set_stream(None)
    r.render("STD"); r.snapshot("on the context's stream")


def _keep_compare(r):
    r.render("STD"); r.snapshot("kept")
    r.keep_views()
    r.set_params(1)
    r.render("STD"); r.snapshot("re-rendered")
    r.compare_views()


def _stream_behind_render(method, yuv):
    def body(r):
        r.render(method); r.snapshot("parameters 0, enqueued before the stream")
        r.set_params(1)
        r.render(method); r.snapshot("parameters 1: its weights are the ones the stream's first copy overwrites")
        r.render_stream(method, yuv)
    return body


SCRIPTS = [
    Script("params_war_std", G8, _params_war("STD")),
    Script("params_war_ten_p3", G8P, _params_war("TEN_WM")),
    Script("params_four_renders_std", G8, _params_four("STD", True)),
    Script("params_four_renders_ten_p3", G8P, _params_four("TEN_WM", True)),
    Script("params_four_back_to_back_std", G9, _params_four("STD", False)),
    Script("params_four_back_to_back_ten_p3", G8P, _params_four("TEN_WM", False)),
    Script("focus_side_stream", G8, _focus_side_stream),
    Script("focus_side_stream_9x9", G9, _focus_side_stream),
    *[Script("write_" + n, G8, _writer(n)) for n in ("upload_image_async", "upload_images_yuv420", "upload_images_yuv_host", "upload_images_yuv_device",
                                                      "upload_mosaic_yuv_device", "upload_mosaic", "fill_synthetic", "fill_synthetic_images",
                                                      "fill_synthetic_scene")],
    Script("write_upload_image_async_9x9_planar", G9P, _writer("upload_image_async")),
    Script("write_attached_grid", G8, _writer("attached_grid_write"), attached=True),
    Script("write_upload_images_yuv_derived", G8, _writer("upload_images_yuv_derived"), released=True),
    Script("write_upload_mosaic_yuv_derived", G8P, _writer("upload_mosaic_yuv_derived"), released=True),
    Script("write_focus_upload_image_async", G8, _writer_focus("upload_image_async")),
    Script("write_focus_fill_synthetic_images", G8, _writer_focus("fill_synthetic_images")),
    Script("rows_int", G8, _int_rows),
    Script("rows_float", G8, _float_rows),
    Script("rows_view_maps", G8, _view_maps),
    Script("switch_stream", G8, _switch, caller=True),
    Script("switch_stream_filter_pending", G8, _switch_filter, caller=True),
    Script("switch_stream_uploads_pending", G8, _switch_uploads, caller=True),
    Script("keep_compare", G8, _keep_compare),
    Script("render_stream_std", G8, _stream_behind_render("STD", False)),
    Script("render_stream_ten", G8, _stream_behind_render("TEN_WM", False)),
    Script("render_stream_yuv420_std", G8, _stream_behind_render("STD", True)),
]
BY_NAME = {s.name: s for s in SCRIPTS}
assert len(BY_NAME) == len(SCRIPTS)


def dry(L, oc, script):
    r = Rec(L, oc, script)
    script.body(r)
    return r


_dry_memo = {}


def dry_cached(L, oc, script):
    if script.name not in _dry_memo:
        _dry_memo[script.name] = dry(L, oc, script)
    return _dry_memo[script.name]


def distinguishability(L, oc, script, floor=0.5):
    """On the CPU, from the oracle alone: every snapshot differs from every state it could be confused with in at least `floor` of its
    colour bytes.  Returns the smallest fraction seen and how many pairs were compared."""
    r = dry_cached(L, oc, script)
    assert r.snapshots, "a script without a snapshot checks nothing"
    worst, pairs = 1.0, 0
    for label, s, alts in r.confusable():
        assert alts, (script.name, label, "nothing to confuse it with")
        for t in alts:
            d = r.oracle.distinct(s, t)
            assert d >= floor, (script.name, label, "could pass as", t, "differs in only", d)
            worst, pairs = min(worst, d), pairs + 1
    if r.map_state is not None:
        m0, m1 = r.final_maps()
        d = float((m0[..., 0] != m1[..., 0]).mean())
        assert d >= floor, (script.name, "map 0 and map 1 differ in only", d)
        worst = min(worst, d)
    if r.compare is not None:
        d = r.oracle.distinct(*r.compare)
        assert d >= floor, (script.name, "the kept and the re-rendered views differ in only", d)
        worst = min(worst, d)
    for kind, method, g, h, _ in r.streamed:
        # the render enqueued last before the stream reads the weight arrays the stream's copies overwrite, block after block
        path, (label, last) = r.oracle.path(h), r.snapshots[-1]
        for b in range(0, PATH_VIEWS, V):
            block = oc.blend_std(r.grids[g], path.focused_offsets, path.offsets, np.ascontiguousarray(path.weights[b:b + V]), threads=8)[..., :3].astype(np.int32)
            d = float((np.abs(block - r.oracle.colour(last)[:block.shape[0]].astype(np.int32)) > 2 * TEN_TOL_LSB).mean())
            assert d >= floor, (script.name, label, "could pass as a render with the stream's weights of block", b // V, d)
            worst, pairs = min(worst, d), pairs + 1
    return worst, pairs


# ---- the live run ------------------------------------------------------------------------------------------------------------------------------

_cycles_per_ms = [None]


def cycles_per_ms(torch):
    """torch.cuda._sleep spins for a number of clock ticks: calibrated once per process with events"""
    if _cycles_per_ms[0] is None:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda._sleep(1_000_000)       # warm
        n = 20_000_000
        a.record()
        torch.cuda._sleep(n)
        b.record()
        b.synchronize()
        _cycles_per_ms[0] = n / a.elapsed_time(b)
    return _cycles_per_ms[0]


class Live:
    """One script on one context: set up, an un-stalled pass (every first-use allocation, the host time to issue), then the stalled pass."""

    def __init__(self, L, oc, script, placement):
        import torch
        self.torch, self.L, self.oc, self.script, self.placement = torch, L, oc, script, placement
        geo = script.geo
        self.plan = dry_cached(L, oc, script)
        self.keep = []
        ctx = self.ctx = L.Context(0)
        ctx.set_grid(geo.cols, geo.rows, W, H)
        if geo.layout != "rgba":
            ctx.set_output_layout(geo.layout)
        self.A = self.plan.grids[0]
        self.grid_t = None
        if script.attached:
            self.grid_t = torch.from_numpy(self.A.copy()).to("cuda:0")
            self.A_t = self.grid_t.clone()
            torch.cuda.synchronize()
            ctx.attach_grid(self.grid_t.data_ptr(), self.grid_t.numel())
            ctx.grid_modified()       # announced once: from now on the derived copies are used
        else:
            ctx.upload_grid(self.A)
        ctx.set_params(self.plan.oracle.hps[self.plan.last_param])
        self.info = ctx.view_layout()
        nbytes = V * self.info.view_stride_bytes
        self.views_t = torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0")
        self.snaps = [torch.zeros(nbytes, dtype=torch.uint8, device="cuda:0") for _ in self.plan.snapshots]
        torch.cuda.synchronize()
        ctx.attach_views(self.views_t.data_ptr(), nbytes)
        if script.released:
            ctx.prepare("TEN_WM")
            ctx.release_inputs()
        own, copy, aux = (torch.cuda.ExternalStream(h) for h in ctx.debug_streams())
        self.streams = {"own": own, "copy": copy, "aux": aux}
        self.other = None
        if script.caller:
            # the caller's streams: a second context's own two (torch's come from a pool of 32 created at once, which fills every hardware queue)
            self.other = L.Context(0)
            s1, s2, _ = self.other.debug_streams()
            self.streams["s1"], self.streams["s2"] = torch.cuda.ExternalStream(s1), torch.cuda.ExternalStream(s2)
        fb = yuv_ref.sizes(W, H)[2]
        self.stream_out = [ctx.pinned_empty((PATH_VIEWS, fb) if kind == "yuv" else (PATH_VIEWS, H, W, 4)) for kind, *_ in self.plan.streamed]
        # the writers' buffers, staged once
        self.staged = []
        for writer, payload, env, _ in self.plan.writes:
            if writer.apply is None:
                new = np.stack([payload["images"][g] for g in range(geo.n)])
                self.staged.append(torch.from_numpy(new).to("cuda:0"))
            else:
                self.staged.append(_stage(L, ctx, writer, payload, env, self.keep))
        torch.cuda.synchronize()
        self.cur = "own"
        self.end = None

    def close(self):
        self.ctx.sync()
        self.torch.cuda.synchronize()
        self.ctx.close()
        if self.other is not None:
            self.other.close()

    # -- steps the recorder hands down --
    def snapshot(self, i):
        with self.torch.cuda.stream(self.streams[self.cur]):
            self.snaps[i].copy_(self.views_t, non_blocking=True)

    def write(self, i):
        s = self.staged[i]
        if isinstance(s, list):
            for name, args, kw in s:
                getattr(self.ctx, name)(*args, **kw)
            return
        with self.torch.cuda.stream(self.streams[self.cur]):      # the caller's write, in the compute stream's order, then announced
            self.grid_t.copy_(s, non_blocking=True)
        self.ctx.grid_modified()

    def set_stream(self, which):
        self.ctx.set_stream(self.streams[which].cuda_stream if which else None)
        self.cur = which or "own"

    # -- a pass --
    def _reset(self, poison):
        ctx, torch = self.ctx, self.torch
        ctx.set_stream(None)
        self.cur = "own"
        ctx.set_params(self.plan.oracle.hps[self.plan.last_param])     # in place; clears the per-view rows
        if self.grid_t is not None:
            self.grid_t.copy_(self.A_t)
            torch.cuda.synchronize()
            ctx.grid_modified()
        else:
            for g in range(self.script.geo.n):
                ctx.upload_image(g, self.A[g])                            # synchronous; after lfi_release_inputs through the staging plane
        ctx.poison(self.L.LFI_POISON_VIEWS | self.L.LFI_POISON_SCRATCH | self.L.LFI_POISON_MAPS | self.L.LFI_POISON_VIEW_MAPS, poison)
        for t in self.snaps:
            t.fill_(poison)
        for a in self.stream_out:
            a[...] = poison
        ctx.sync()
        if self.script.caller:
            self.set_stream("s1")
        ctx.upload_wait()
        torch.cuda.synchronize()

    def _stalled_stream(self):
        if self.placement == "compute":
            return "s1" if self.script.caller else "own"
        return self.placement

    def check_not_drained(self, rec):
        rec.checked_not_drained = True
        done = self.end is not None and self.end.query()
        self.not_drained = not done
        if self.end is not None:
            slow = sorted(rec.calls, key=lambda c: -c[1])[:3]
            assert not done, ("the stall has ended before the last asynchronous call returned: a call blocked the host (or the stall is too short)",
                              "stall ms", self.stall_ms, "slowest calls (ms)", [(c[0], round(c[1] * 1e3, 2)) for c in slow],
                              "all calls (ms)", [(c[0], round(c[1] * 1e3, 2)) for c in rec.calls])

    def run(self):
        torch = self.torch
        # pass 1: un-stalled
        self._reset(POISON[1])
        warm = Rec(self.L, self.oc, self.script, live=self)
        t = time.perf_counter()
        self.script.body(warm)
        issue_ms = (time.perf_counter() - t) * 1e3
        self.ctx.sync()
        torch.cuda.synchronize()
        self.stall_ms = min(max(STALL_FACTOR * issue_ms, STALL_MIN_MS), STALL_MAX_MS)
        # pass 2: stalled
        self._reset(POISON[0])
        stalled = self._stalled_stream()
        self.end = torch.cuda.Event()
        with torch.cuda.stream(self.streams[stalled]):
            torch.cuda._sleep(int(self.stall_ms * cycles_per_ms(torch)))
            self.end.record()
        canaries = []
        for name, s in self.streams.items():
            if name != stalled:
                e = torch.cuda.Event()
                e.record(s)
                canaries.append((name, e))
        t = time.perf_counter()
        while not all(e.query() for _, e in canaries) and (time.perf_counter() - t) * 1e3 < CANARY_MS:
            pass
        isolated = {name: e.query() for name, e in canaries}
        pending = not self.end.query()
        rec = Rec(self.L, self.oc, self.script, live=self)
        t = time.perf_counter()
        self.script.body(rec)
        if not rec.checked_not_drained:
            self.check_not_drained(rec)
        issued_ms = (time.perf_counter() - t) * 1e3
        self.end.synchronize()
        self.ctx.sync()
        torch.cuda.synchronize()
        print(f"stream_order {self.script.name} [{self.placement}]: stall {self.stall_ms:.1f} ms on {stalled}, issue {issue_ms:.2f} ms un-stalled / {issued_ms:.2f} ms stalled")
        assert all(isolated.values()) and pending, ("isolation canary: the streams share a hardware queue with the stalled one — nothing would be proved",
                                                    isolated, "stall pending", pending)
        self._check_bytes(rec)
        return rec

    def _decode(self, t):
        raw = t.cpu().numpy()
        if self.info.layout == self.L.LFI_LAYOUT_RGBA:
            return raw.reshape(V, H, W, 4)
        planes = np.lib.stride_tricks.as_strided(raw, (V, 3, H, W), (self.info.view_stride_bytes, self.info.plane_stride_bytes, self.info.row_pitch_bytes, 1))
        out = np.full((V, H, W, 4), 255, np.uint8)
        out[..., :3] = planes.transpose(0, 2, 3, 1)
        return out

    def _check_bytes(self, rec):
        for i, (label, st) in enumerate(rec.snapshots):
            check_views(self._decode(self.snaps[i]), rec.oracle.views(st), st.method, (self.script.name, self.placement, "snapshot", i, label))
        maps = rec.final_maps()
        if maps is not None:
            for k in (0, 1):
                got = self.ctx.download_map(k)
                assert (got == maps[k]).all(), (self.script.name, self.placement, "final map", k, int((got != maps[k]).any(-1).sum()))
        if rec.view_maps_made is not None:
            want = rec.oracle.view_maps(*rec.view_maps_made)
            for v in range(V):
                for k in (0, 1):
                    assert (self.ctx.download_view_map(v, k) == want[v][k]).all(), (self.script.name, self.placement, "view", v, "map", k)
        for i, (kind, method, _, _, out) in enumerate(rec.streamed):
            want = rec.streamed_want(i)
            if kind == "yuv":
                assert (out == want).all(), (self.script.name, self.placement, "streamed YUV frames differ", int((out != want).sum()))
            else:
                check_views(out, want, method, (self.script.name, self.placement, "streamed views"))
        if rec.compare is not None:
            a, b = (rec.oracle.colour(s).astype(np.int64) for s in rec.compare)
            per_view, _ = rec.compared
            for v in range(V):
                assert per_view[v].differing_bytes == int((a[v] != b[v]).sum()) > 0, (self.script.name, "compare_views: differing bytes of view", v)
                assert list(per_view[v].sq_err) == [int(((a[v, ..., c] - b[v, ..., c]) ** 2).sum()) for c in range(3)], (self.script.name, "sq_err of view", v)


# ---- the child process -------------------------------------------------------------------------------------------------------------------------
# tests/test_gpu_stream_order.py runs this file once, in a fresh process with eight hardware queues: the stream-switch scripts use five streams
# (the context's three and the caller's two) beside the null stream, and with the runtime's default of four queues the caller's second
# stream shares a queue with the first — the canary then fails the case, as it must.  One JSON line per case; nothing after a case that ended
# in anything but an assertion.

def main(argv):
    import json
    import lfinterpolator_amd as L
    from oracle import lfi_oracle_c as oc
    oc.build()
    oc.lib()
    t_all = time.perf_counter()
    for script in SCRIPTS:
        if argv and script.name not in argv:
            continue
        for placement in PLACEMENTS:
            t, live, res = time.perf_counter(), None, {"script": script.name, "placement": placement, "ok": False, "message": "", "fatal": False}
            try:
                live = Live(L, oc, script, placement)
                live.run()
                res["ok"] = True
            except AssertionError as e:
                res["message"] = str(e)[:2000]
            except Exception as e:      # a HIP error: nothing more is started on the device
                res["message"], res["fatal"] = f"{type(e).__name__}: {e}"[:2000], True
            if live is not None:
                res["stall_ms"] = getattr(live, "stall_ms", None)
                if not res["fatal"]:
                    live.close()
            res["seconds"] = round(time.perf_counter() - t, 3)
            print("RESULT " + json.dumps(res), flush=True)
            if res["fatal"]:
                return 1
    print(f"TOTAL {time.perf_counter() - t_all:.1f} s", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
