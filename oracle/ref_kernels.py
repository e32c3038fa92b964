"""ctypes binding of oracle/_ref/libref_kernels.so — the reference's OWN kernels (its src/kernels.cu, unchanged), compiled for the
CPU over the shim headers in oracle/ref_shim/ and run by oracle/ref_kernels.cpp (`make -C oracle ref`).  TEST INFRASTRUCTURE ONLY: the
checker of the oracle itself; nothing under lfinterpolator_amd/ loads it.

`fused=True` is the library built with -ffp-contract=fast (nvcc's default --fmad=true); `fused=False` the one built with
-ffp-contract=off, which exists only to show that a test can tell the two apart.

The arguments are the oracle's: lf [N][H][W][4] u8, focused [N][2] int32, offsets [N][2] float32, weights [64][N] fp16 bits.  All-focus
launches take BOTH maps and the kernel picks the one it reads (Standard::process<true>: map 1, Tensors::process<true>: map 0)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = {True: os.path.join(_HERE, "_ref", "libref_kernels.so"), False: os.path.join(_HERE, "_ref", "libref_kernels_nofma.so")}
SELFTEST = os.path.join(_HERE, "_ref", "ref_selftest")
_libs = {}


def ref_root() -> str:
    """Where the reference tree is looked for: $REF, as in oracle/Makefile, or its default."""
    return os.environ.get("REF", "/root/reference")


def tree_present() -> bool:
    return os.path.isfile(os.path.join(ref_root(), "src", "kernels.cu"))


def _make(target: str) -> subprocess.CompletedProcess:
    return subprocess.run(["make", "-C", _HERE, "REF=" + ref_root(), target], check=False, capture_output=True, text=True)


def available(build: bool = True) -> bool:
    """True when both libraries exist (they are built on demand where the reference tree is present)."""
    if build and tree_present():
        _make("ref")
    return all(os.path.exists(p) for p in _SO.values())


def selftest() -> subprocess.CompletedProcess:
    """Build and run the stand-alone self-test (the driver with its own main under the host sanitizers)."""
    return _make("ref-selftest")


_vp = C.c_void_p
_i32p = C.POINTER(C.c_int32)


def lib(fused: bool = True):
    if fused not in _libs:
        if not available():
            raise RuntimeError("oracle/_ref/libref_kernels*.so are missing (make -C oracle ref needs the reference tree)")
        l = C.CDLL(_SO[fused])
        l.ref_last_error.restype = C.c_char_p
        l.ref_contracts.restype = C.c_int
        blend = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, _vp, C.c_int, _vp, _vp, C.c_float, C.c_float, _vp]
        l.ref_std.restype = l.ref_ten.restype = C.c_int
        l.ref_std.argtypes = l.ref_ten.argtypes = blend
        l.ref_estimate.restype = C.c_int
        l.ref_estimate.argtypes = [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _vp, _vp, C.c_int, C.c_float, C.c_float, _i32p, _vp]
        l.ref_filter.restype = C.c_int
        l.ref_filter.argtypes = [_vp, C.c_int, C.c_int, _i32p, _vp]
        assert l.ref_contracts() == int(fused)
        _libs[fused] = l
    return _libs[fused]


class Refused(ValueError):
    """The launch is one the reference's kernels cannot do (the message says why)."""


def _check(l, rc):
    if rc != 0:
        raise Refused(l.ref_last_error().decode())


def _p(a):
    return None if a is None else a.ctypes.data_as(_vp)


def _blend(name, lf, cols, rows, focused, offsets, weights, all_focus, map0, map1, focus, rng, fused):
    lf = np.ascontiguousarray(lf, np.uint8)
    n, h, w, _ = lf.shape
    assert n == cols * rows
    foc = np.ascontiguousarray(focused, np.int32)
    off = np.ascontiguousarray(offsets, np.float32)
    wv = np.ascontiguousarray(weights, np.uint16)
    assert foc.shape == (n, 2) and off.shape == (n, 2) and wv.ndim == 2 and wv.shape[1] == n
    maps = [None if m is None else np.ascontiguousarray(m, np.uint8) for m in (map0, map1)]
    assert all(m is None or m.shape == (h, w, 4) for m in maps)
    out = np.zeros((64, h, w, 4), np.uint8)
    l = lib(fused)
    _check(l, getattr(l, name)(_p(lf), cols, rows, w, h, wv.shape[0], _p(foc), _p(off), _p(wv), int(all_focus), _p(maps[0]), _p(maps[1]),
                               focus, rng, _p(out)))
    return out


def blend_std(lf, cols, rows, focused, offsets, weights, all_focus=False, map0=None, map1=None, focus=0.0, rng=0.0, fused=True):
    """Standard::process<all_focus>: [64][H][W][4]."""
    return _blend("ref_std", lf, cols, rows, focused, offsets, weights, all_focus, map0, map1, focus, rng, fused)


def blend_ten(lf, cols, rows, focused, offsets, weights, all_focus=False, map0=None, map1=None, focus=0.0, rng=0.0, fused=True):
    """Tensors::process<all_focus>, its mma_sync modelled as the oracle's M16 (oracle/ref_shim/mma.h): [64][H][W][4]."""
    return _blend("ref_ten", lf, cols, rows, focused, offsets, weights, all_focus, map0, map1, focus, rng, fused)


def focus_estimate(lf, cols, rows, offsets, ids, focus, rng, radius, fused=True):
    """FocusMap::estimate: map 0, [H][W][4]."""
    lf = np.ascontiguousarray(lf, np.uint8)
    n, h, w, _ = lf.shape
    assert n == cols * rows
    off = np.ascontiguousarray(offsets, np.float32)
    ids = np.ascontiguousarray(ids, np.int32)
    radius = np.ascontiguousarray(radius, np.int32)
    out = np.zeros((h, w, 4), np.uint8)
    l = lib(fused)
    _check(l, l.ref_estimate(_p(lf), cols, rows, w, h, _p(off), _p(ids), len(ids), focus, rng, radius.ctypes.data_as(_i32p), _p(out)))
    return out


def focus_filter(map0, radius, fused=True):
    """FocusMap::filter: map 1 from map 0, [H][W][4]."""
    map0 = np.ascontiguousarray(map0, np.uint8)
    h, w = map0.shape[:2]
    radius = np.ascontiguousarray(radius, np.int32)
    out = np.zeros((h, w, 4), np.uint8)
    l = lib(fused)
    _check(l, l.ref_filter(_p(map0), w, h, radius.ctypes.data_as(_i32p), _p(out)))
    return out
