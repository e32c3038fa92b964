"""Every way the inputs of a context change (WRITERS) against every call that reads a derived copy of them (READERS).

A context keeps three derived copies of its inputs: the planar copy of the fixed-focus renders (ensure_planar, csrc/hip/lfi_dispatch.hpp:
planar_version, img_version[], grid_full_version, planar_reach), the padded planes of the focus estimate (launch_focus_factored_keys,
csrc/hip/lfi_focus_sched.hpp: pad_version, pad_ids, pad_shift, pad_radius, slot reuse under lfi_view_focus_maps), and, after
lfi_release_inputs, the planar copy as the only copy.  Whether a reader sees the current inputs rests on a touch_all / touch_images call at
every writer.  A stale plane renders a plausible picture of the previous frame, so nothing but a comparison with the right answer shows it.

This file is the table both tests walk: tests/test_input_writers_table.py (CPU: the header's writer family is covered, and no (writer,
reader) pair could pass on a stale copy) and tests/test_gpu_input_writers.py (GPU: every pair, on a context whose copies were built before
the write).  It imports without a GPU.

A writer is one ABI call (or the few calls that make one step) with the images it changes.  Its host side — what the grid holds afterwards —
comes from the restatements under tests/ alone (yuv_in_ref, yuv_left_ref, yuv10_ref, yuv_surfaces_ref, mosaic_ref) and the oracle's
synthetic_lf, never from the device.  lfi_fill_synthetic_scene had no restatement: scene_lf below is one, written from the header's text and
the formula in the comment above fill_scene (csrc/hip/focus_map.hpp).

A reader is held to the CPU oracle on the shadow grid: STD renders, focus maps, per-view maps and focus curves byte for byte, TEN_WM as
fuzz_cases.fuzz_blend holds it (within one LSB of M16 and inside the interval of the exact sum, tests/ten_interval.py); the flagged
fixed-focus renders (LFI_FLAG_DEEP_VIEWS, LFI_FLAG_IN_FRAME, LFI_FLAG_LINEAR_LIGHT) as fuzz_cases.fuzz_flagged holds them.

Limits: at these shapes a missing stream wait may go unobserved — the copies take microseconds.  The tests hold the version bookkeeping
and the routing; they do not hold the races.  tests/stream_order.py does: every asynchronous writer here is issued there behind a stalled stream.
"""
import hashlib
from dataclasses import dataclass

import numpy as np

import deep_ref
import derived_ref
import focus_curve_ref as fref
import focus_steps_ref
import inframe_ref
import linear_ref
import mosaic_ref as mref
import ten_interval
import view_rows
import yuv10_ref
import yuv_in_ref as in_ref
import yuv_left_ref as left_ref
import yuv_surfaces_ref as sref
from oracle.lfi_oracle_np import _fma32, _mix32

F32 = np.float32
TRAJ = "0.071,0.071,0.93,0.93"
VIEWS, FOCUS, RANGE, EFFECT, ASPECT = 4, 0.22, 0.17, 3.0, 1.783
FOCUS_LARGE = 0.9          # a set_params that grows planar_reach and pad_shift
RAMP = (0.05, 0.4)         # the focus ramp of the per-view integer rows
TILES = (3, 2)             # focus_tiles
TEN_TOL_LSB = 1            # as fuzz_cases.TEN_TOL_LSB
POISON = (0xA5, 0x5A)


@dataclass(frozen=True)
class Shape:
    name: str
    cols: int
    rows: int
    W: int
    H: int
    ids: int        # 0: every id build_params selects; else the first `ids` of them — then some images are not sampled by the focus readers
    radius2: tuple  # the other block radius of the state changer

    @property
    def n(self):
        return self.cols * self.rows

    @property
    def rect(self):
        """focus_curve's rectangle: ragged on every side"""
        return (self.W // 5, self.H // 4, self.W - self.W // 3, self.H - self.H // 5)


# the smallest shapes at which the machinery is live; even sizes (the YUV writers).  136 is a multiple of 8 and not of 128; 130 is no multiple
# of 4: the YUV kernels' rows16 = false and the mosaic kernels' UNALIGNED routes
SHAPES = [Shape("g4x4_136x24", 4, 4, 136, 24, 0, (4, 2)), Shape("g3x5_130x18", 3, 5, 130, 18, 8, (4, 2))]


# ---- the shadow: the inputs and parameters of a context, carried on the host ----------------------------------------------------------------

@dataclass
class Shadow:
    shape: Shape
    grid: np.ndarray           # [N][H][W][4] uint8
    focus: float = FOCUS
    rng: float = RANGE
    radius: tuple = None       # None: build_params'
    steps: int = 32            # lfi_set_focus_steps
    layout: str = "rgba"
    siting: str = "centre"     # lfi_set_yuv_siting's in_siting
    released: bool = False
    views: int = VIEWS         # lfi_params.views (tests/context_reuse.py takes a context from one view count to another)
    wide: bool = False         # the weight column of image N // 2 is 2.5: outside [0, 2), weights_scalable is false

    def params(self, L):
        s = self.shape
        hp = L.build_params(s.cols, s.rows, s.W, s.H, TRAJ, self.focus, self.rng, EFFECT, ASPECT, self.views)
        if s.ids:
            hp.focus_map_ids = hp.focus_map_ids[:s.ids].copy()
        if self.wide:
            hp.weights = hp.weights.copy()
            hp.weights[:, s.n // 2] = 0x4100     # fp16 2.5
        if self.radius is not None:
            hp.block_radius = np.array(self.radius, np.int32)
        return hp

    def view_ids(self, L):
        s = self.shape
        ids = L.build_view_focus_ids(s.cols, s.rows, TRAJ, self.views)
        return np.ascontiguousarray(ids[:, :s.ids] if s.ids else ids)

    def key(self):
        return (self.shape.name, self.shape.ids, hashlib.sha1(self.grid.tobytes()).hexdigest(), self.focus, self.rng, self.radius, self.steps, self.views, self.wide)


def first_grid(oc, shape):
    """inputs A of every test"""
    return oc.synthetic_lf(shape.n, shape.W, shape.H, 0x1F1F)


def random_images(n, shape, seed):
    out = np.random.default_rng(seed).integers(0, 256, (n, shape.H, shape.W, 4), dtype=np.uint8)
    out[..., 3] = 255
    return out


def scene_lf(offsets, n, W, H, seed, focus, rng):
    """lfi_fill_synthetic_scene in numpy: image g shows the texture T of 8 x 8-pixel cells at (x − floor(f*·offset_g.x), y − floor(f*·offset_g.y)),
    f* one of the estimate's candidates 3, 11, 20, 28 of [focus, focus + range] per 1024 x 1024-pixel block; the product in float32"""
    y, x = np.meshgrid(np.arange(H, dtype=np.int64), np.arange(W, dtype=np.int64), indexing="ij")
    out = np.empty((n, H, W, 4), np.uint8)
    with np.errstate(over="ignore"):
        level = _mix32(np.uint32(seed) ^ ((x >> 10).astype(np.uint32) * np.uint32(73856093)) ^ ((y >> 10).astype(np.uint32) * np.uint32(19349663))) & np.uint32(3)
        k = (np.uint32(3) + np.uint32(8) * level + (level >> np.uint32(1))).astype(F32)
        fs = _fma32(F32(F32(rng) / F32(31.0)), k, F32(focus))
        for g in range(n):
            u = x - np.floor(fs * F32(offsets[g, 0])).astype(np.int64)
            v = y - np.floor(fs * F32(offsets[g, 1])).astype(np.int64)
            cell = _mix32(_mix32(np.uint32(seed) + (u >> 3).astype(np.uint32) * np.uint32(0x9E3779B9)) + (v >> 3).astype(np.uint32) * np.uint32(0x85EBCA6B))
            for c in range(3):
                out[g, ..., c] = (cell >> np.uint32(8 * c)) & np.uint32(0xFF)
    out[..., 3] = 255
    return out


# ---- writers ------------------------------------------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class Env:
    """what a writer's host side may depend on: the shape, a seed, the context's input siting and its current parameters"""
    L: object
    oc: object
    shape: Shape
    seed: int
    siting: str
    hp: object


@dataclass(frozen=True)
class Writer:
    name: str
    abi: tuple          # the functions of include/lfi.h this row stands for
    runs: object        # n -> [(g0, g1), …]: the runs of images it changes; None: the whole grid
    make: object        # Env -> payload: {"images": {g: [H][W][4]}, …} — the new images from the restatements, and the bytes to hand to the call
    apply: object       # (L, ctx, payload, env, keep) -> None: the call(s); keep: a list that holds buffers alive as long as the context
    released: bool = False   # runs on a context after lfi_release_inputs
    torch: bool = False      # needs torch for device memory

    def image_runs(self, n):
        return [(0, n)] if self.runs is None else self.runs(n)

    def images(self, n):
        return [g for g0, g1 in self.image_runs(n) for g in range(g0, g1)]


def shadow_apply(grid, payload, writer, skip_run=None):
    """the grid after the writer; skip_run: the index of one run left unapplied (a stale plane)"""
    out = grid.copy()
    runs = writer.image_runs(grid.shape[0])
    assert sorted(payload["images"]) == writer.images(grid.shape[0]), (writer.name, sorted(payload["images"]))
    for g, image in payload["images"].items():
        if skip_run is not None and runs[skip_run][0] <= g < runs[skip_run][1]:
            continue
        out[g] = image
    return out


def _place(ctx, flat, memory, keep):
    """the bytes in page-locked host memory or in device memory (a torch tensor: 256-byte aligned); its address"""
    flat = np.ascontiguousarray(flat, np.uint8).reshape(-1)
    if memory == sref.DEVICE:
        import torch
        t = torch.from_numpy(flat.copy()).to("cuda:0")
        torch.cuda.synchronize()   # torch's stream and the context's know nothing of each other
        assert t.data_ptr() % 16 == 0
        keep.append(t)
        return t.data_ptr()
    a = ctx.pinned_empty((flat.size,))
    a[...] = flat
    keep.append(a)
    return a.ctypes.data


def _siting(env, forced=None):
    return (forced or env.siting) == "left"


def _yuv8(runs, fmt, layout, memory, conv, via420=False, forced_siting=None, derived=False):
    """lfi_upload_images_yuv (or lfi_upload_images_yuv420, or lfi_upload_images_yuv_derived) of 8-bit frames, one call per run"""
    def make(env):
        s, images, calls = env.shape, {}, []
        ref = left_ref if _siting(env, forced_siting) else in_ref
        for i, (g0, g1) in enumerate(runs(s.n)):
            frames = np.random.default_rng(env.seed + 31 * i).integers(0, 256, (g1 - g0, in_ref.sizes(s.W, s.H)[2]), dtype=np.uint8)
            for k, image in enumerate(ref.images(frames, s.W, s.H, *conv)):
                images[g0 + k] = image
            calls.append((g0, frames))
        return {"images": images, "calls": calls}

    def apply(L, ctx, p, env, keep):
        s = env.shape
        if forced_siting:
            ctx.set_yuv_siting(forced_siting, "centre")
        for g0, frames in p["calls"]:
            if via420:
                keep.append(frames)
                ctx.upload_images_yuv420(frames, g0, matrix=conv[0], range=conv[1], chroma=conv[2])
                continue
            lay = layout(fmt, s.W, s.H)
            base = _place(ctx, sref.scatter(frames, lay, 0xEE), memory, keep)
            desc = sref.descriptor(L, lay, memory, base, keep=keep)
            if memory == sref.DEVICE:
                assert all(v % 16 == 0 for v in (base, lay.frame_stride, lay.y_pitch, lay.c_offset, lay.c_pitch, lay.cr_offset)), "not read in place"
            (ctx.upload_images_yuv_derived if derived else ctx.upload_images_yuv)(desc, frames.shape[0], g0, matrix=conv[0], range=conv[1], chroma=conv[2])
        if forced_siting:
            ctx.set_yuv_siting(env.siting, "centre")

    return make, apply


def _p010(runs, conv):
    def make(env):
        s, images, calls = env.shape, {}, []
        for i, (g0, g1) in enumerate(runs(s.n)):
            codes = np.random.default_rng(env.seed + 31 * i).integers(0, 1024, (g1 - g0, yuv10_ref.sizes(s.W, s.H)[2]), dtype=np.uint16)
            junk = np.random.default_rng(env.seed + 5).integers(0, 1 << 16, codes.shape, dtype=np.uint16)
            for k, image in enumerate(yuv10_ref.images(codes, s.W, s.H, conv[0], conv[1], conv[2], yuv10_ref.LEFT if _siting(env) else yuv10_ref.CENTRE)):
                images[g0 + k] = image
            calls.append((g0, codes, junk))
        return {"images": images, "calls": calls}

    def apply(L, ctx, p, env, keep):
        s = env.shape
        lay = yuv10_ref.tight(yuv10_ref.P010, s.W, s.H)
        for g0, codes, junk in p["calls"]:
            base = _place(ctx, yuv10_ref.scatter(codes, lay, 0xEE, junk), sref.HOST, keep)
            ctx.upload_images_yuv(yuv10_ref.descriptor(L, lay, yuv10_ref.HOST, base, keep=keep), codes.shape[0], g0, matrix=conv[0], range=conv[1], chroma=conv[2])

    return make, apply


def _mosaic_yuv(geometry, fmt, layout, memory, conv, derived=False):
    """geometry: shape -> (tiles_x, tiles_y, order, bottom_up, first_tile, n, g0)"""
    def make(env):
        s = env.shape
        tiles_x, tiles_y, order, bottom_up, first_tile, n, g0 = geometry(s)
        mw, mh = tiles_x * s.W, tiles_y * s.H
        frame = np.random.default_rng(env.seed).integers(0, 256, in_ref.sizes(mw, mh)[2], dtype=np.uint8)
        tiles = mref.mosaic_map(tiles_x, tiles_y, first_tile, n, mref.GRID if order == "grid" else mref.ROWS, mref.BOTTOM_UP if bottom_up else 0, s.cols, s.rows, g0)
        assert tiles is not None, geometry(s)
        return {"images": mref.expand(frame, mw, mh, s.W, s.H, tiles, conv[0], conv[1], conv[2], _siting(env)), "frame": frame}

    def apply(L, ctx, p, env, keep):
        s = env.shape
        tiles_x, tiles_y, order, bottom_up, first_tile, n, g0 = geometry(s)
        lay = layout(fmt, tiles_x * s.W, tiles_y * s.H)
        base = _place(ctx, sref.scatter(p["frame"][None], lay, 0xEE), memory, keep)
        desc = sref.descriptor(L, lay, memory, base, keep=keep)
        if memory == sref.DEVICE:
            assert all(v % 16 == 0 for v in (base, lay.y_pitch, lay.c_offset, lay.c_pitch, lay.cr_offset)), "not read in place"
        call = ctx.upload_mosaic_yuv_derived if derived else ctx.upload_mosaic_yuv
        call(L.Mosaic.make(tiles_x, tiles_y, order, bottom_up, first_tile, n), desc, g0, matrix=conv[0], range=conv[1], chroma=conv[2])

    return make, apply


def _rgba(runs, how):
    """random RGBA images into the runs; how(ctx, g, image, keep): the call for one image"""
    def make(env):
        images = {}
        for i, (g0, g1) in enumerate(runs(env.shape.n)):
            for k, image in enumerate(random_images(g1 - g0, env.shape, env.seed + 31 * i)):
                images[g0 + k] = image
        return {"images": images}

    def apply(L, ctx, p, env, keep):
        for g, image in p["images"].items():
            how(ctx, g, image, keep)

    return make, apply


def _upload_async_pinned(ctx, g, image, keep):
    a = ctx.pinned_empty(image.shape)
    a[...] = image
    keep.append(a)
    ctx.upload_image_async(g, a)


def _upload_async_pageable(ctx, g, image, keep):
    ctx.upload_image_async(g, np.ascontiguousarray(image))   # staged by the runtime: free on return


def _make_synthetic(runs):
    def make(env):
        lf = env.oc.synthetic_lf(env.shape.n, env.shape.W, env.shape.H, env.seed)
        return {"images": {g: lf[g] for g0, g1 in runs(env.shape.n) for g in range(g0, g1)}, "seed": env.seed}
    return make


def _make_scene(env):
    s = env.shape
    lf = scene_lf(env.hp.offsets, s.n, s.W, s.H, env.seed, env.hp.focus, env.hp.range)
    return {"images": {g: lf[g] for g in range(s.n)}, "seed": env.seed}


def _make_mosaic_rgba(env):
    s = env.shape
    tiles_x, tiles_y, first_tile, n, g0 = 2, 2, 1, 3, 0
    image = np.random.default_rng(env.seed).integers(0, 256, (tiles_y * s.H, tiles_x * s.W + 5, 4), dtype=np.uint8)   # a row pitch beyond the tiles
    image[..., 3] = 255
    tiles = mref.mosaic_map(tiles_x, tiles_y, first_tile, n, mref.ROWS, 0, s.cols, s.rows, g0)
    return {"images": mref.rgba_tiles(image, s.W, s.H, tiles), "image": image}


def _apply_mosaic_rgba(L, ctx, p, env, keep):
    keep.append(p["image"])
    ctx.upload_mosaic(L.Mosaic.make(2, 2, "rows", first_tile=1, n=3), p["image"], 0)


def _make_whole(env):
    return {"images": dict(enumerate(random_images(env.shape.n, env.shape, env.seed)))}


def _build_copies(ctx):
    """the planar copy and the estimate's padded planes from what the planes hold NOW, unchecked — so that the write that follows meets
    copies that only its own lfi_grid_modified can invalidate (lfi_attach_grid and lfi_grid_device_ptr move the versions themselves, but
    they came before the copies)"""
    ctx.render("TEN_WM")
    ctx.focus_tiles(*TILES)   # the factored estimate's planes, and no map written: a reader may have been set up before the writer
    ctx.sync()                # the write below is not on the context's stream


def _apply_attach(L, ctx, p, env, keep):
    """a caller-owned buffer that holds other bytes is attached and announced once (from then on the copies are used), the copies are built
    from it; then the device write and its announcement"""
    import torch
    new = np.stack([p["images"][g] for g in range(env.shape.n)])
    t = torch.from_numpy(np.bitwise_xor(new, np.uint8(0x80))).to("cuda:0")
    torch.cuda.synchronize()
    keep.append(t)
    ctx.attach_grid(t.data_ptr(), t.numel())
    ctx.grid_modified()
    _build_copies(ctx)
    t.copy_(torch.from_numpy(new))           # the device write, on torch's stream
    torch.cuda.synchronize()
    ctx.grid_modified()


def _apply_raw_pointer(L, ctx, p, env, keep):
    """a write through lfi_grid_device_ptr behind the context's back — by a second context that took the pointer as an attached grid — announced
    by lfi_grid_modified"""
    s = env.shape
    ptr, nbytes = ctx.grid_device_ptr()
    ctx.grid_modified()        # announced once: from now on the copies are used, and only a further announcement refreshes them
    _build_copies(ctx)
    other = L.Context(0)
    other.set_grid(s.cols, s.rows, s.W, s.H)
    other.attach_grid(ptr, nbytes)
    for g, image in p["images"].items():
        other.upload_image(g, image)     # synchronous
    other.close()
    ctx.grid_modified()


def _single(n):
    return [(3, 4)]


def _middle(n):
    return [(5, 9)]


def _two_runs(n):
    return [(1, 2), (7, 9)]


def _tail(n):
    return [(n - 3, n)]


def _head(n):
    return [(0, 5)]


def _both_ends(n):
    return [(0, 2), (n - 2, n)]


def _last_two(n):
    return [(n - 2, n)]


C709 = (in_ref.BT709, in_ref.LIMITED, in_ref.BILINEAR)
C601F = (in_ref.BT601, in_ref.FULL, in_ref.BILINEAR)
C709N = (in_ref.BT709, in_ref.FULL, in_ref.NEAREST)
RELEASE = "lfi_release_inputs"


def _w(name, abi, runs, make_apply, **kw):
    return Writer(name, abi, runs, make_apply[0], make_apply[1], **kw)


WRITERS = [
    _w("upload_grid", ("lfi_upload_image",), None, _rgba(lambda n: [(0, n)], lambda ctx, g, im, keep: ctx.upload_image(g, im))),
    _w("upload_image", ("lfi_upload_image",), _single, _rgba(_single, lambda ctx, g, im, keep: ctx.upload_image(g, im))),
    _w("upload_image_async_pageable", ("lfi_upload_image_async",), _two_runs, _rgba(_two_runs, _upload_async_pageable)),
    _w("upload_image_async_pinned", ("lfi_upload_image_async",), _tail, _rgba(_tail, _upload_async_pinned)),
    _w("fill_synthetic", ("lfi_fill_synthetic",), None, (_make_synthetic(lambda n: [(0, n)]), lambda L, ctx, p, env, keep: ctx.fill_synthetic(p["seed"]))),
    _w("fill_synthetic_partial", ("lfi_fill_synthetic_images",), _head, (_make_synthetic(_head), lambda L, ctx, p, env, keep: ctx.fill_synthetic(p["seed"], 0, 5))),
    _w("fill_synthetic_scene", ("lfi_fill_synthetic_scene",), None, (_make_scene, lambda L, ctx, p, env, keep: ctx.fill_synthetic_scene(p["seed"]))),
    _w("upload_images_yuv420", ("lfi_upload_images_yuv420",), _middle, _yuv8(_middle, sref.I420, sref.tight, sref.HOST, C709, via420=True)),
    _w("upload_images_yuv_i420_host", ("lfi_upload_images_yuv",), _both_ends, _yuv8(_both_ends, sref.I420, sref.tight, sref.HOST, C601F)),
    _w("upload_images_yuv_nv12_host_pitched", ("lfi_upload_images_yuv",), lambda n: [(2, 6)], _yuv8(lambda n: [(2, 6)], sref.NV12, sref.pitched, sref.HOST, C709N)),
    _w("upload_images_yuv_nv12_device_in_place", ("lfi_upload_images_yuv",), lambda n: [(6, n)], _yuv8(lambda n: [(6, n)], sref.NV12, sref.pitched, sref.DEVICE, C709), torch=True),
    _w("upload_images_yuv_p010_host", ("lfi_upload_images_yuv",), lambda n: [(9, 12)], _p010(lambda n: [(9, 12)], C709)),
    _w("upload_images_yuv_left_sited", ("lfi_upload_images_yuv", "lfi_set_yuv_siting"), lambda n: [(4, 7)],
       _yuv8(lambda n: [(4, 7)], sref.I420, sref.pitched, sref.HOST, C709, forced_siting="left")),
    _w("upload_mosaic_yuv_rows", ("lfi_upload_mosaic_yuv",), lambda n: [(10, 14)],
       _mosaic_yuv(lambda s: (3, 2, "rows", False, 1, 4, 10), sref.I420, sref.tight, sref.HOST, C709)),
    _w("upload_mosaic_yuv_grid", ("lfi_upload_mosaic_yuv",), None,
       _mosaic_yuv(lambda s: (s.cols, s.rows, "grid", True, 0, s.n, 0), sref.NV12, sref.pitched, sref.HOST, C601F)),
    _w("upload_mosaic_yuv_device_in_place", ("lfi_upload_mosaic_yuv",), lambda n: [(n - 8, n)],
       _mosaic_yuv(lambda s: (4, 2, "rows", False, 0, 8, s.n - 8), sref.I420, sref.pitched, sref.DEVICE, C709), torch=True),
    _w("upload_mosaic", ("lfi_upload_mosaic",), lambda n: [(0, 3)], (_make_mosaic_rgba, _apply_mosaic_rgba)),
    _w("attach_grid_write_modified", ("lfi_attach_grid", "lfi_grid_modified"), None, (_make_whole, _apply_attach), torch=True),
    _w("grid_device_ptr_write_modified", ("lfi_grid_device_ptr", "lfi_grid_modified", "lfi_attach_grid"), _last_two, (_rgba(_last_two, None)[0], _apply_raw_pointer)),
    # after lfi_release_inputs: the planar copy is the only copy of the inputs
    _w("released_upload_image", (RELEASE, "lfi_upload_image"), lambda n: [(2, 3)], _rgba(lambda n: [(2, 3)], lambda ctx, g, im, keep: ctx.upload_image(g, im)), released=True),
    _w("released_upload_images_yuv_derived", (RELEASE, "lfi_upload_images_yuv_derived"), lambda n: [(3, 6)],
       _yuv8(lambda n: [(3, 6)], sref.NV12, sref.pitched, sref.HOST, C709, derived=True), released=True),
    _w("released_upload_mosaic_yuv_derived", (RELEASE, "lfi_upload_mosaic_yuv_derived"), None,
       _mosaic_yuv(lambda s: (s.cols, s.rows, "grid", False, 0, s.n, 0), sref.I420, sref.tight, sref.HOST, C709, derived=True), released=True),
]

# functions of the header's writer family that have no row, each with its reason
EXCLUDED = {
    "lfi_broadcast_grid": "refuses two contexts on one device (\"the contexts of a broadcast must sit on distinct devices\"): tests/test_distributed.py runs it",
    "lfi_upload_wait": "waits for the copy stream; writes nothing",
    "lfi_upload_map": "writes focus maps 0 / 1, not inputs: no derived copy depends on it",
    "lfi_upload_view_map": "writes a view's focus maps, not inputs: no derived copy depends on it",
}
WRITER_FAMILY = r"lfi_upload_\w*|lfi_fill_\w*|lfi_attach_grid|lfi_grid_modified|lfi_grid_device_ptr|lfi_broadcast_grid|lfi_release_inputs"


# ---- readers ------------------------------------------------------------------------------------------------------------------------------------

_memo = {}


def _cached(kind, s, fn):
    k = (kind,) + s.key()
    if k not in _memo:
        if len(_memo) > 400:
            _memo.clear()
        _memo[k] = fn()
    return _memo[k]


def _the_map(shape):
    """the uploaded map of the all-focus reader: every focus byte occurs"""
    return view_rows.random_maps(shape.H, shape.W, 5)[0]


def _pixel_costs(L, s):
    hp = s.params(L)
    return _cached("costs", s, lambda: fref.pixel_costs(s.grid, hp.offsets, hp.focus_map_ids, hp.focus, hp.range, hp.block_radius, 32))


def _view_offsets(L, s):
    sh = s.shape
    D = L.build_view_offsets(sh.cols, sh.rows, sh.W, sh.H, TRAJ, ASPECT, L.focus_ramp(RAMP[0], RAMP[1], s.views))
    O, _ = L.build_view_centred_offsets(sh.cols, sh.rows, sh.W, sh.H, TRAJ, ASPECT, np.full(s.views, s.focus, np.float32))
    return D, O


def _layout(ctx, s, layout, fixed):
    """the per-writer tests name each fixed-focus reader's view layout; the long-lived sequence renders in whatever layout its steps left"""
    if fixed and s.layout != layout:
        ctx.set_output_layout(layout)
        s.layout = layout


_poisons = [0]


def _byte():
    _poisons[0] += 1
    return POISON[_poisons[0] & 1]


class Reader:
    """want(oc, L, s, ctx=None): the oracle's answer on the shadow; prepare(L, ctx, s, fixed): what may happen BEFORE the writer (the view
    layout, per-view rows, the poison of what the read writes — never LFI_POISON_DERIVED or LFI_POISON_FOCUS_WORKSPACE: they reset
    grid_version and pad_version, the bookkeeping under test); read(L, ctx, s): the call and its downloads; check(got, want): assertions;
    done(ctx): per-view rows cleared.  focus: the reader samples the focus ids alone."""
    name = ""
    released = False   # applies after lfi_release_inputs too
    focus = False
    variant = None

    def sampled(self, L, s):
        """the images the reader's output depends on"""
        if not self.focus:
            return set(range(s.shape.n))
        return {int(g) for g in s.params(L).focus_map_ids}

    def prepare(self, L, ctx, s, fixed=True):
        pass

    def done(self, ctx):
        pass

    def flat(self, want):
        """the want as a list of arrays, for the stale-copy self-check"""
        return [np.asarray(w) for w in (want if isinstance(want, (list, tuple)) else [want])]


class Std(Reader):
    name, released = "std_rgba_layout", True

    def want(self, oc, L, s, ctx=None):
        hp = s.params(L)
        return _cached("std", s, lambda: oc.blend_std(s.grid, hp.focused_offsets, hp.offsets, hp.weights, threads=8))

    def prepare(self, L, ctx, s, fixed=True):
        _layout(ctx, s, "rgba", fixed)
        ctx.set_variant("STD", "auto")
        ctx.poison(L.LFI_POISON_VIEWS, _byte())

    def read(self, L, ctx, s):
        ctx.render("STD")
        return ctx.download_views()

    def check(self, got, want):
        assert (got == want).all(), ("STD", int((got != want).sum()), np.argwhere((got != want).any(axis=(1, 2, 3))).ravel().tolist())


class TenPlanar(Reader):
    name, released = "ten_wm_planar_layout", True

    def want(self, oc, L, s, ctx=None):
        hp = s.params(L)

        def compute():
            lo, hi = ten_interval.bounds(oc, s.grid, hp, threads=8)
            return oc.blend_ten(s.grid, hp.focused_offsets, hp.offsets, hp.weights, model=oc.TEN_M16, threads=8), lo, hi
        return _cached("ten", s, compute)

    def prepare(self, L, ctx, s, fixed=True):
        _layout(ctx, s, "planar", fixed)
        ctx.set_variant("TEN_WM", "auto")
        ctx.poison(L.LFI_POISON_VIEWS, _byte())

    def read(self, L, ctx, s):
        ctx.render("TEN_WM")
        return ctx.download_views(), ctx.last_kernel_name()

    def check(self, got, want):
        (views, kernel), (m16, lo, hi) = got, want
        d = int(np.abs(views.astype(int) - m16.astype(int)).max())
        out = ten_interval.outside(views, lo, hi)
        assert d <= TEN_TOL_LSB and out == 0, ("TEN_WM", kernel, "lsb", d, "outside the interval", out)

    def flat(self, want):
        return [want[0]]


class ViewRows(Reader):
    name = "view_rows_planar_source"

    def want(self, oc, L, s, ctx=None):
        hp, sh = s.params(L), s.shape
        D = _view_offsets(L, s)[0].copy()
        D[..., 0], D[..., 1] = np.clip(D[..., 0], -sh.W, sh.W), np.clip(D[..., 1], -sh.H, sh.H)
        return _cached("rows", s, lambda: np.stack([oc.blend_std(s.grid, np.ascontiguousarray(D[v]), hp.offsets, hp.weights[v:v + 1])[0] for v in range(s.views)]))

    def prepare(self, L, ctx, s, fixed=True):
        _layout(ctx, s, "rgba", fixed)
        ctx.set_view_offsets(_view_offsets(L, s)[0])
        ctx.poison(L.LFI_POISON_VIEWS, _byte())

    def read(self, L, ctx, s):
        ctx.render("STD")
        return ctx.download_views(), ctx.last_kernel_name()

    def check(self, got, want):
        views, kernel = got
        assert kernel == view_rows.KERNEL["int", "planar"].format("STD"), kernel
        assert (views == want).all(), ("per-view rows", int((views != want).sum()), np.argwhere((views != want).any(axis=(1, 2, 3))).ravel().tolist())

    def done(self, ctx):
        ctx.set_view_offsets(None)


class AllFocus(Reader):
    name = "all_focus_std_uploaded_map"

    def want(self, oc, L, s, ctx=None):
        hp, m = s.params(L), _the_map(s.shape)
        return _cached("af", s, lambda: oc.blend_std(s.grid, hp.focused_offsets, hp.offsets, hp.weights, all_focus=True, map_plane=m, focus=hp.focus, rng=hp.range, threads=8))

    def prepare(self, L, ctx, s, fixed=True):
        _layout(ctx, s, "rgba", fixed)
        ctx.set_variant("STD", "auto")
        for k in (0, 1):
            ctx.upload_map(k, _the_map(s.shape))
        ctx.poison(L.LFI_POISON_VIEWS, _byte())

    def read(self, L, ctx, s):
        ctx.render("STD", all_focus=True)
        return ctx.download_views()

    def check(self, got, want):
        assert (got == want).all(), ("all-focus STD", int((got != want).sum()))


def _want_maps(oc, L, s, offsets, ids, steps):
    hp = s.params(L)
    if steps == 32:
        m0 = oc.focus_estimate(s.grid, offsets, ids, hp.focus, hp.range, hp.block_radius, threads=8)
    else:
        m0 = focus_steps_ref.map0(s.grid, offsets, ids, hp.focus, hp.range, hp.block_radius, steps)
    return m0, oc.focus_filter(m0, hp.block_radius, threads=8)


class FocusMap(Reader):
    focus = True

    def __init__(self, variant):
        self.variant, self.name = variant, "focus_map_" + variant

    def want(self, oc, L, s, ctx=None):
        hp = s.params(L)
        return _cached("maps", s, lambda: _want_maps(oc, L, s, hp.offsets, hp.focus_map_ids, s.steps))

    def prepare(self, L, ctx, s, fixed=True):
        ctx.set_variant("FOCUS", self.variant)
        ctx.poison(L.LFI_POISON_MAPS, _byte())

    def read(self, L, ctx, s):
        ctx.focus_map()
        return ctx.download_map(0), ctx.download_map(1)

    def check(self, got, want):
        for k in (0, 1):
            assert (got[k] == want[k]).all(), (self.name, "map", k, int((got[k] != want[k]).any(-1).sum()))


class ViewFocusMaps(Reader):
    """lfi_view_focus_maps for four views, then lfi_focus_map at once: the pad slots the views reused are handed back"""
    name, focus = "view_focus_maps_then_focus_map", True

    def sampled(self, L, s):
        return {int(g) for g in s.view_ids(L).ravel()} | {int(g) for g in s.params(L).focus_map_ids}

    def want(self, oc, L, s, ctx=None):
        hp, ids, O = s.params(L), s.view_ids(L), _view_offsets(L, s)[1]

        def compute():
            out = []
            for v in range(s.views):
                out += list(_want_maps(oc, L, s, np.ascontiguousarray(O[v]), np.ascontiguousarray(ids[v]), 32))   # the per-view maps keep 32 candidates
            return out + list(_want_maps(oc, L, s, hp.offsets, hp.focus_map_ids, s.steps))
        return _cached("view_maps", s, compute)

    def prepare(self, L, ctx, s, fixed=True):
        ctx.set_variant("FOCUS", "factored")
        ctx.set_view_float_offsets(_view_offsets(L, s)[1])
        ctx.poison(L.LFI_POISON_VIEW_MAPS | L.LFI_POISON_MAPS, _byte())

    def read(self, L, ctx, s):
        ctx.view_focus_maps(s.view_ids(L))
        ctx.focus_map()
        out = []
        for v in range(s.views):
            out += [ctx.download_view_map(v, 0), ctx.download_view_map(v, 1)]
        return out + [ctx.download_map(0), ctx.download_map(1)]

    def check(self, got, want):
        for i, (g, w) in enumerate(zip(got, want)):
            what = ("view", i // 2, "map", i % 2) if i < len(got) - 2 else ("lfi_focus_map behind the views", "map", i % 2)
            assert (g == w).all(), (what, int((g != w).any(-1).sum()))

    def done(self, ctx):
        ctx.set_view_float_offsets(None)


class FocusTiles(Reader):
    name, focus = "focus_tiles_3x2", True

    def want(self, oc, L, s, ctx=None):
        costs, sh = _pixel_costs(L, s), s.shape
        cost = np.stack([np.stack([fref.curve(costs, *L.focus_tile_rect(sh.W, sh.H, TILES[0], TILES[1], tx, ty)) for tx in range(TILES[0])]) for ty in range(TILES[1])])
        return cost, np.argmin(cost, axis=-1).astype(np.int32)

    def read(self, L, ctx, s):
        cost, best, focus = ctx.focus_tiles(*TILES)
        assert (focus == L.focus_candidates(s.focus, s.rng, 32)[best]).all()
        return cost, best

    def check(self, got, want):
        assert (got[0] == want[0]).all(), ("focus_tiles cost", int((got[0] != want[0]).sum()))
        assert (got[1] == want[1]).all(), ("focus_tiles best_index", got[1].tolist(), want[1].tolist())


class FocusCurve(Reader):
    name, focus = "focus_curve_rectangle", True

    def want(self, oc, L, s, ctx=None):
        cost = fref.curve(_pixel_costs(L, s), *s.shape.rect)
        return cost, np.int32(fref.first_min(cost))

    def read(self, L, ctx, s):
        cost, best, focus = ctx.focus_curve(*s.shape.rect)
        assert focus == L.focus_candidates(s.focus, s.rng, 32)[best]
        return cost, np.int32(best)

    def check(self, got, want):
        assert (got[0] == want[0]).all(), ("focus_curve cost", int((got[0] != want[0]).sum()))
        assert got[1] == want[1], ("focus_curve best_index", int(got[1]), int(want[1]))


@dataclass
class _CpuLayout:
    """a layout of the planar copy for the CPU self-check: the GPU test asks the context for its own"""
    pitch_bytes: int
    rows: int
    padx: int


class Derived(Reader):
    """lfi_debug_download_derived after lfi_release_inputs: every byte of the only copy, padding included (tests/derived_ref.py)"""
    name, released = "download_derived", True

    def want(self, oc, L, s, ctx=None):
        if ctx is None:
            return derived_ref.planes(s.grid, _CpuLayout(s.shape.W + 64, s.shape.H, 32), np.arange(s.shape.n) % 16)
        lay = ctx.derived_layout()
        return derived_ref.planes(s.grid, lay, lay.phases)

    def read(self, L, ctx, s):
        return ctx.download_derived()

    def check(self, got, want):
        assert (got == want).all(), ("the planar copy", int((got != want).sum()), np.argwhere((got != want).any(axis=(1, 2, 3))).ravel().tolist())


class Flagged(Reader):
    """a fixed-focus render under a parameter flag (launch_flagged_views, which has its own copy of the join_uploads / ensure_planar /
    set_planar_args sequence): deep_blend, blend_inframe or blend_linear from the planar copy, before and after lfi_release_inputs.  prepare
    sets the shadow's parameters with the flag — before the writer — and the planar view layout, which the flags need whatever the steps
    left; done puts the parameters back without it.  The want is the reference tests/fuzz_cases.py::fuzz_flagged holds the kernels to:
    deep STD bytes and codes `==` the oracle's chain, in-frame and linear-light STD `==` their restatements, linear-light TEN_WM inside the
    interval of the exact sum"""
    released = True
    KERNEL = {deep_ref.FLAG_DEEP_VIEWS: "deep_blend", inframe_ref.FLAG_IN_FRAME: "blend_inframe", linear_ref.FLAG_LINEAR_LIGHT: "blend_linear"}

    def __init__(self, name, flag, method):
        self.name, self.flag, self.method = name, flag, method
        self.deep = flag == deep_ref.FLAG_DEEP_VIEWS
        self._hp = None

    def want(self, oc, L, s, ctx=None):
        hp = s.params(L)

        def compute():
            if self.deep:
                out, pre = oc.blend_std(s.grid, hp.focused_offsets, hp.offsets, hp.weights, return_prequant=True, threads=8)
                return out[..., :3], deep_ref.q10_std(pre)
            if self.flag == inframe_ref.FLAG_IN_FRAME:
                return (inframe_ref.restate(s.grid, hp).bytes,)
            res = linear_ref.restate(s.grid, hp)
            return (res.bytes,) if self.method == "STD" else linear_ref.ten_interval_of(res, hp, s.shape.n) + (res.bytes,)
        return _cached(self.name, s, compute)

    def flat(self, want):
        """the stale-copy self-check compares bytes a render would write (TEN_WM: the restatement's, which lie inside the interval), not bounds"""
        return [np.asarray(w) for w in (want[2:] if self.method == "TEN_WM" else want)]

    def prepare(self, L, ctx, s, fixed=True):
        if s.layout != "planar":
            ctx.set_output_layout("planar")
            s.layout = "planar"
        self._hp = s.params(L)
        ctx.set_params(self._hp, flags=self.flag)
        ctx.poison(L.LFI_POISON_VIEWS | (L.LFI_POISON_DEEP if self.deep else 0), _byte())   # (the deep planes: where an earlier read left them)

    def read(self, L, ctx, s):
        ctx.render(self.method)
        return ctx.download_views(), ctx.download_deep_views() if self.deep else None, ctx.last_kernel_name()

    def check(self, got, want):
        views, codes, kernel = got
        assert kernel == f"{self.KERNEL[self.flag]}<{self.method}>", kernel
        assert (views[..., 3] == 255).all(), (self.name, "alpha")
        c = views[..., :3]
        if self.method == "TEN_WM":
            lo, hi, _ = want
            out = int(((c < lo) | (c > hi)).sum())
            assert out == 0, (self.name, "bytes outside the interval", out)
            return
        assert (c == want[0]).all(), (self.name, int((c != want[0]).sum()), np.argwhere((c != want[0]).any(axis=(1, 2, 3))).ravel().tolist())
        if self.deep:
            assert (codes == want[1]).all(), (self.name, "codes", int((codes != want[1]).sum()))

    def done(self, ctx):
        if self._hp is not None:
            ctx.set_params(self._hp)
            self._hp = None


READERS = [Std(), TenPlanar(), ViewRows(), AllFocus(), FocusMap("factored"), FocusMap("factored_direct"), FocusMap("plain"), ViewFocusMaps(),
           FocusTiles(), FocusCurve(), Derived(),
           Flagged("deep_std", deep_ref.FLAG_DEEP_VIEWS, "STD"), Flagged("inframe_std", inframe_ref.FLAG_IN_FRAME, "STD"),
           Flagged("linear_std", linear_ref.FLAG_LINEAR_LIGHT, "STD"), Flagged("linear_ten", linear_ref.FLAG_LINEAR_LIGHT, "TEN_WM")]
FLAGGED_READERS = [r for r in READERS if isinstance(r, Flagged)]


def readers_of(writer_or_released):
    """the readers that apply: after lfi_release_inputs the fixed-focus renders, flagged ones included, and the copy itself; else all but the copy's download
    (lfi_debug_download_derived serves a current copy only, and whether it is current is what the renders show)"""
    released = writer_or_released.released if isinstance(writer_or_released, Writer) else bool(writer_or_released)
    return [r for r in READERS if (r.released if released else r.name != "download_derived")]


def pairs():
    """every (writer, reader) pair the GPU test executes"""
    return [(w, r) for w in WRITERS for r in readers_of(w)]


# ---- the stale-copy self-check (CPU, oracle only) ---------------------------------------------------------------------------------------------------

def differs(reader, a, b):
    return any(not np.array_equal(x, y) for x, y in zip(reader.flat(a), reader.flat(b)))


def stale_copy_check(oc, L, shape, writer, seed=1):
    """For every reader of the writer: its expected output after the writer must differ from the one before — and, for a partial writer, from
    the one with any single run left unapplied — or a stale plane would pass.  The exception: images the reader does not sample (a focus reader
    and a run outside the focus ids) MUST leave it unchanged.  Returns [(reader name, what, must change)] of every comparison made."""
    before = Shadow(shape, first_grid(oc, shape))
    env = Env(L, oc, shape, seed, "centre", before.params(L))
    payload = writer.make(env)
    after = Shadow(shape, shadow_apply(before.grid, payload, writer))
    runs = writer.image_runs(shape.n)
    assert not np.array_equal(before.grid, after.grid)
    for g0, g1 in runs:
        assert all(not np.array_equal(before.grid[g], after.grid[g]) for g in range(g0, g1)), (writer.name, "an image of the run keeps its bytes")
    table = []
    for reader in readers_of(writer):
        want = reader.want(oc, L, after)
        stale = [("nothing applied", before.grid, set(writer.images(shape.n)))]
        if len(runs) > 1:
            stale += [(f"run {runs[i]} left unapplied", shadow_apply(before.grid, payload, writer, skip_run=i), set(range(*runs[i]))) for i in range(len(runs))]
        for what, grid, missing in stale:
            must = bool(missing & reader.sampled(L, after))
            changed = differs(reader, want, reader.want(oc, L, Shadow(shape, grid)))
            assert changed == must, (writer.name, reader.name, what, "the expected output " + ("does not change: a stale copy would pass" if must else "changes although no sampled image did"))
            table.append((reader.name, what, must))
    return table
