"""The orientation kernel on the CPU (no GPU): every workgroup of csrc/orient_band.hpp's body, lane by lane with the kernel's barrier
(tests/emu/emu_orient.cpp), against the numpy statement (tests/orient_ref.py) — and every destination byte stored exactly once, none
outside the image, no unaligned dword.  The window mapping of the same header against orient_ref.source_window.

The checks are plain functions over the emulation library (`build`); tests/test_orient.py's one test runs them all, beside the checks
of the statement and of the EXIF reader, and reports every one that fails."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import orient_ref as OR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EMU = os.path.join(ROOT, "tests", "emu")
_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-DJPGPU_HOST_EMULATION"]


def build(tmp_dir):
    """tests/emu/emu_orient.cpp as a shared library in tmp_dir (g++, the flags of tests/emu/Makefile) -> the ctypes library."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    assert cxx is not None, "no C++ compiler"
    so = os.path.join(str(tmp_dir), "libemuorient.so")
    subprocess.check_call([cxx, *_FLAGS, "-shared", "-I", _EMU, "-include", os.path.join(_EMU, "hip_shim.hpp"), "-o", so, os.path.join(_EMU, "emu_orient.cpp")])
    L = C.CDLL(so)
    u, p = C.c_uint32, C.c_void_p
    L.emu_orient.argtypes = [p, u, u, u, u, p, p]
    L.emu_orient.restype = u
    L.emu_orient_tile.restype = u
    L.emu_orient_window.argtypes = [u] * 7 + [p]
    L.emu_orient_window.restype = C.c_int
    return L


def _aligned(n, fill):
    """n bytes at a 4-byte aligned address, with room to the next multiple of 4 behind them (the arena's contract), filled."""
    raw = np.full(n + 16, fill, np.uint8)
    at = (-raw.ctypes.data) % 4
    return raw, raw[at:at + n]


def _run(L, src, o):
    h, w, nc = src.shape
    n = h * w * nc
    sraw, s = _aligned(n, 0xEE)
    s[:] = src.reshape(-1)
    draw, d = _aligned(n, 0x5A)
    count = np.zeros(n, np.uint32)
    outside = L.emu_orient(s.ctypes.data, w, h, nc, o, d.ctypes.data, count.ctypes.data)
    assert outside == 0, (w, h, nc, o, outside)
    assert (draw[:(-draw.ctypes.data) % 4] == 0x5A).all() and (draw[(-draw.ctypes.data) % 4 + n:] == 0x5A).all()  # (nothing around the image)
    return d.copy(), count


def _sizes(T):
    edge = [(h, w) for h in (T - 1, T, T + 1) for w in (T - 1, T, T + 1)]
    return [(1, 1), (1, 37), (37, 1), (3, 2 * T + 5), (2 * T + 5, 3)] + edge


def every_workgroup_against_the_numpy_statement_every_byte_stored_once(emu, nc):
    T = emu.emu_orient_tile()
    rng = np.random.default_rng(100 + nc)
    for (h, w) in _sizes(T):
        src = rng.integers(0, 256, (h, w, nc), dtype=np.uint8)
        for o in range(1, 9):
            got, count = _run(emu, src, o)
            want = OR.orient(src, o)
            assert want.shape[:2] == ((w, h) if o >= 5 else (h, w))
            assert (count == 1).all(), (h, w, nc, o, int((count == 0).sum()), int((count > 1).sum()))
            assert np.array_equal(got, want.reshape(-1)), (h, w, nc, o)


def more_than_two_tiles_a_side(emu):
    T = emu.emu_orient_tile()
    rng = np.random.default_rng(7)
    src = rng.integers(0, 256, (2 * T + 9, 3 * T + 2, 3), dtype=np.uint8)
    for o in range(1, 9):
        got, count = _run(emu, src, o)
        assert (count == 1).all() and np.array_equal(got, OR.orient(src, o).reshape(-1)), o


def window_mapping_is_the_reference_rule(emu):
    rng = np.random.default_rng(3)
    out = (C.c_uint32 * 6)()
    for _ in range(400):
        w, h = int(rng.integers(1, 300)), int(rng.integers(1, 300))
        o = int(rng.integers(1, 9))
        ow, oh = OR.oriented_size(o, w, h)
        x, y = int(rng.integers(0, ow)), int(rng.integers(0, oh))
        ww, wh = int(rng.integers(1, ow - x + 1)), int(rng.integers(1, oh - y + 1))
        assert emu.emu_orient_window(o, w, h, x, y, ww, wh, out) == 0
        sx, sy, sw, sh = OR.source_window(o, w, h, (x, y, ww, wh))
        assert tuple(out) == (sx, sy, sw, sh, ow, oh)
        # the mapping means: the window of O is the orientation of that window of S
        a = rng.integers(0, 256, (h, w, 1), dtype=np.uint8)
        assert np.array_equal(OR.orient(a, o)[y:y + wh, x:x + ww], OR.orient(a[sy:sy + sh, sx:sx + sw], o))
        assert emu.emu_orient_window(o, w, h, x, y, ow - x + 1, wh, out) == -1 and emu.emu_orient_window(o, w, h, x, y, ww, oh - y + 1, out) == -1
    assert emu.emu_orient_window(6, 10, 20, 0, 0, 0, 0, out) == 0 and tuple(out) == (0, 0, 0, 0, 20, 10)
    with pytest.raises(ValueError):
        OR.source_window(6, 10, 20, (0, 0, 11, 21))


def checks(emu):
    """(name, callable) of every check of this file."""
    out = [(f"emulation, {nc} channel(s)", lambda nc=nc: every_workgroup_against_the_numpy_statement_every_byte_stored_once(emu, nc)) for nc in (1, 3, 4)]
    return out + [("emulation, more than two tiles a side", lambda: more_than_two_tiles_a_side(emu)),
                  ("window mapping of orient_band.hpp", lambda: window_mapping_is_the_reference_rule(emu))]
