"""Surfaces of include/lfi.h's lfi_yuv_surfaces in numpy: a layout (format, pitches, plane offsets, frame stride), tight I420 frames
scattered into surfaces of that layout and gathered back.  Every byte the frames do not own — pitch padding, the gaps between planes and
frames — holds a poison value the caller chooses.  The expected BYTES come from tests/yuv_ref.py and tests/yuv_in_ref.py as they are; this
file only says where they lie."""
from dataclasses import dataclass

import numpy as np

I420, NV12 = 0, 1          # LFI_YUV_I420, LFI_YUV_NV12
HOST, DEVICE = 0, 1        # LFI_MEM_HOST, LFI_MEM_DEVICE


def sizes(w, h):
    """(cw, ch, frame_bytes)"""
    cw, ch = (w + 1) >> 1, (h + 1) >> 1
    return cw, ch, w * h + 2 * cw * ch


@dataclass(frozen=True)
class Layout:
    fmt: int
    w: int
    h: int
    y_pitch: int
    c_offset: int
    c_pitch: int
    cr_offset: int
    frame_stride: int

    @property
    def extent(self):
        """the end of a frame's last plane"""
        ch = (self.h + 1) >> 1
        return (self.c_offset if self.fmt == NV12 else self.cr_offset) + ch * self.c_pitch


def _up(v, a):
    return (v + a - 1) // a * a


def tight(fmt, w, h):
    """what lfi_yuv_surfaces_packed describes"""
    cw, ch, fb = sizes(w, h)
    return Layout(fmt, w, h, w, w * h, 2 * cw if fmt == NV12 else cw, 0 if fmt == NV12 else w * h + cw * ch, fb)


def pitched(fmt, w, h, align=256, gap=256, tail=256):
    """a decoder's surface: pitches rounded up to `align`, `gap` bytes between the Y plane and the chroma (and between Cb and Cr), `tail`
    bytes behind the frame"""
    cw, ch, _ = sizes(w, h)
    y_pitch = _up(w, align)
    c_pitch = _up(2 * cw if fmt == NV12 else cw, align)
    c_offset = h * y_pitch + gap
    cr_offset = 0 if fmt == NV12 else c_offset + ch * c_pitch + gap
    end = (c_offset if fmt == NV12 else cr_offset) + ch * c_pitch
    return Layout(fmt, w, h, y_pitch, c_offset, c_pitch, cr_offset, end + tail)


def own_mask(lay):
    """[frame_stride] bool: the bytes of a frame that carry data"""
    cw, ch, _ = sizes(lay.w, lay.h)
    m = np.zeros(lay.frame_stride, bool)
    for y in range(lay.h):
        m[y * lay.y_pitch:y * lay.y_pitch + lay.w] = True
    for y in range(ch):
        if lay.fmt == NV12:
            m[lay.c_offset + y * lay.c_pitch:lay.c_offset + y * lay.c_pitch + 2 * cw] = True
        else:
            for off in (lay.c_offset, lay.cr_offset):
                m[off + y * lay.c_pitch:off + y * lay.c_pitch + cw] = True
    return m


def scatter(frames, lay, poison, out=None):
    """[n][frame_stride] uint8: tight I420 frames [n][frame_bytes] in surfaces of layout lay; every other byte is `poison`"""
    frames = np.asarray(frames, np.uint8)
    n = frames.shape[0]
    cw, ch, fb = sizes(lay.w, lay.h)
    assert frames.shape[1] >= fb
    if out is None:
        out = np.empty((n, lay.frame_stride), np.uint8)
    out[...] = poison
    for k in range(n):
        y = frames[k, :lay.w * lay.h].reshape(lay.h, lay.w)
        cb = frames[k, lay.w * lay.h:lay.w * lay.h + cw * ch].reshape(ch, cw)
        cr = frames[k, lay.w * lay.h + cw * ch:fb].reshape(ch, cw)
        for r in range(lay.h):
            out[k, r * lay.y_pitch:r * lay.y_pitch + lay.w] = y[r]
        for r in range(ch):
            if lay.fmt == NV12:
                row = out[k, lay.c_offset + r * lay.c_pitch:lay.c_offset + r * lay.c_pitch + 2 * cw]
                row[0::2], row[1::2] = cb[r], cr[r]
            else:
                out[k, lay.c_offset + r * lay.c_pitch:lay.c_offset + r * lay.c_pitch + cw] = cb[r]
                out[k, lay.cr_offset + r * lay.c_pitch:lay.cr_offset + r * lay.c_pitch + cw] = cr[r]
    return out


def gather(surfaces, lay):
    """[n][frame_bytes] uint8: the tight I420 frames of surfaces [n][>= extent]"""
    surfaces = np.asarray(surfaces, np.uint8)
    n = surfaces.shape[0]
    cw, ch, fb = sizes(lay.w, lay.h)
    out = np.empty((n, fb), np.uint8)
    for k in range(n):
        y = out[k, :lay.w * lay.h].reshape(lay.h, lay.w)
        cb = out[k, lay.w * lay.h:lay.w * lay.h + cw * ch].reshape(ch, cw)
        cr = out[k, lay.w * lay.h + cw * ch:].reshape(ch, cw)
        for r in range(lay.h):
            y[r] = surfaces[k, r * lay.y_pitch:r * lay.y_pitch + lay.w]
        for r in range(ch):
            if lay.fmt == NV12:
                row = surfaces[k, lay.c_offset + r * lay.c_pitch:lay.c_offset + r * lay.c_pitch + 2 * cw]
                cb[r], cr[r] = row[0::2], row[1::2]
            else:
                cb[r] = surfaces[k, lay.c_offset + r * lay.c_pitch:lay.c_offset + r * lay.c_pitch + cw]
                cr[r] = surfaces[k, lay.cr_offset + r * lay.c_pitch:lay.cr_offset + r * lay.c_pitch + cw]
    return out


def padding_holds(surfaces, lay, poison):
    """every byte outside the planes' own bytes still holds the poison"""
    surfaces = np.asarray(surfaces, np.uint8)
    return bool((surfaces[:, ~own_mask(lay)[:surfaces.shape[1]]] == poison).all())


def descriptor(native, lay, memory, base, keep=None):
    """the lfi_yuv_surfaces of layout lay at address base"""
    return native.YuvSurfaces.make(lay.fmt, memory, base, lay.frame_stride, lay.y_pitch, lay.c_offset, lay.c_pitch, lay.cr_offset, keep=keep)
