"""CPU emulation of the window kernel (csrc/window_band.hpp) against the oracle's whole decode, sliced.

tests/emu/emu_window.cpp compiles the product's planner and kernel phases with g++ (the flags of tests/emu/Makefile) and runs
every workgroup of the launch grid; a window's bytes must equal `full.reshape(H, W, nc)[y:y+h, x:x+w]` (interleaving colour
functions), `full.reshape(H, nc, W)[y:y+h, :, x:x+w]` (ColorTransform None) or `full.reshape(H, W)[y:y+h, x:x+w]` (one
component).  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import oracle as O
import synth

import jpeg_decoder_amd as J  # (host-side structs only)

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_CSRC = os.path.join(os.path.dirname(_HERE), "jpeg-decoder_amd", "csrc")
# the flags of tests/emu/Makefile
_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-DJPGPU_HOST_EMULATION"]
GEOM_WORDS = 128


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("emu_window")
    so = str(d / "libemuwin.so")
    cmd = [os.environ.get("CXX", "g++"), *_FLAGS, "-shared", "-I", _EMU, "-include", os.path.join(_EMU, "hip_shim.hpp"), "-o", so,
           os.path.join(_EMU, "emu_window.cpp"), os.path.join(_CSRC, "image_job.cpp")]
    subprocess.check_call(cmd)
    L = C.CDLL(so)
    L.emu_window_plan.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_size_t]
    L.emu_window_plan.restype = C.c_int
    L.emu_window_tile_blocks.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p]
    L.emu_window_tile_blocks.restype = C.c_int
    L.emu_window_decode.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.POINTER(C.c_size_t)]
    L.emu_window_decode.restype = C.c_int
    return L


def _to_j(ocomps):
    out = (J.Component * len(ocomps))()
    for i, c in enumerate(ocomps):
        out[i].identifier, out[i].horizontal_sampling_factor, out[i].vertical_sampling_factor = c.identifier, c.h, c.v
        out[i].quantization_table_index, out[i].dct_scale = c.tq, c.dct_scale
        out[i].size_width, out[i].size_height, out[i].block_width, out[i].block_height = c.size_w, c.size_h, c.block_w, c.block_h
    return out


def grid_of(ocomps, ow, oh):
    return (ocomps[0].size_w, ocomps[0].size_h) if len(ocomps) == 1 else (ow, oh)


def window_slice(full, W, H, nc, ct, win):
    x, y, w, h = win
    if nc == 1:
        return full.reshape(H, W)[y:y + h, x:x + w].reshape(-1)
    if ct.upper() == "NONE":
        return full.reshape(H, nc, W)[y:y + h, :, x:x + w].reshape(-1)
    return full.reshape(H, W, nc)[y:y + h, x:x + w].reshape(-1)


def windows_for(W, H, seed):
    """The whole image, 1x1 at the four corners, interior windows with x % 8 != 0 and odd w, windows ending on the right and
    bottom edges, edges on tile boundaries (multiples of 8 / 16 / 64) and on odd chroma columns / rows, seeded random ones."""
    cand = [(0, 0, W, H), (0, 0, 1, 1), (W - 1, 0, 1, 1), (0, H - 1, 1, 1), (W - 1, H - 1, 1, 1),
            (13, 5, W - 20, H - 9), (5, 3, 7, 5), (W - 37, H - 11, 37, 11), (W - 9, 0, 9, H), (0, H - 3, W, 3),
            (16, 8, 48, 16), (64, 16, 65, 33), (128, 32, 33, 17), (33, 17, 31, 15), (3, 1, 2, 2), (1, 1, W - 2, H - 2),
            (W // 2, H // 2, W - W // 2, H - H // 2), (W // 3 | 1, H // 3 | 1, W // 3 | 1, H // 3 | 1)]
    rng = np.random.default_rng(seed)
    for _ in range(4):
        w = int(rng.integers(1, W + 1))
        h = int(rng.integers(1, H + 1))
        cand.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    out = []
    for (x, y, w, h) in cand:
        if x >= 0 and y >= 0 and w > 0 and h > 0 and x + w <= W and y + h <= H and (x, y, w, h) not in out:
            out.append((x, y, w, h))
    return out


LAYOUTS = [
    ([(2, 2), (1, 1), (1, 1)], "YCbCr"), ([(2, 1), (1, 1), (1, 1)], "YCbCr"), ([(1, 2), (1, 1), (1, 1)], "YCbCr"),
    ([(1, 1), (1, 1), (1, 1)], "YCbCr"), ([(1, 1)], "Grayscale"), ([(2, 2)], "Grayscale"), ([(4, 1), (1, 1), (1, 1)], "YCbCr"),
    ([(3, 1), (1, 1), (1, 1)], "YCbCr"), ([(2, 2), (1, 1), (1, 1), (1, 1)], "CMYK"), ([(2, 2), (1, 1), (1, 1), (2, 2)], "YCCK"),
    ([(1, 1)] * 4, "CMYK"), ([(1, 1)] * 3, "RGB"), ([(1, 1)] * 3, "None"), ([(1, 1)] * 4, "None"),
]
SIZES = [(1, 1), (17, 9), (161, 97), (50, 34)]  # (50: 4:2:0 / 4:2:2 chroma 25 columns wide)


def _image(w_, h_, samp, scale, kind, seed):
    rng = np.random.default_rng(seed)
    ocomps, _ = O.make_components(w_, h_, samp, dct_scale=scale)
    ow, oh = J.scaled_output_size(w_, h_, scale)
    if kind == "sparse":
        qts = [rng.integers(1, 64, 64).astype(np.uint16) for _ in ocomps]
        coefs = [synth.sparse_coefficients(rng, c.block_w * c.block_h, amp=64, dc_amp=500) for c in ocomps]
    else:  # hostile: the full-size transform must be the wrap-exact one
        qts = [rng.integers(1, 65536, 64).astype(np.uint16) for _ in ocomps]
        coefs = [rng.integers(-32768, 32768, c.block_w * c.block_h * 64).astype(np.int16) for c in ocomps]
    return ocomps, qts, coefs, ow, oh


def _decode(lib, desc, coefs, win, out_len):
    n = desc.ncomp
    ptrs = (C.c_void_p * n)(*[c.ctypes.data for c in coefs])
    buf = np.full(out_len + 64, 0x5A, np.uint8)  # guard band: the kernel must not write past the window
    ln = C.c_size_t(0)
    w = np.array(win, np.uint32)
    rc = lib.emu_window_decode(C.byref(desc), ptrs, w.ctypes.data, buf.ctypes.data, C.byref(ln))
    return rc, buf, ln.value


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{'_'.join(f'{h}{v}' for h, v in l[0])}-{l[1]}")
@pytest.mark.parametrize("scale", [8, 4, 2, 1])
@pytest.mark.parametrize("kind", ["sparse", "hostile"])
def test_window_kernel_logic_matches_oracle_slice(lib, size, layout, scale, kind):
    samp, ct = layout
    w_, h_ = size
    ocomps, qts, coefs, ow, oh = _image(w_, h_, samp, scale, kind, w_ * 7 + h_ * 131 + scale + len(samp) * 1009 + (kind == "hostile"))
    try:
        full = O.pixels_from_coefficients(ocomps, qts, coefs, ow, oh, ct.upper())
    except O.OracleError:
        pytest.skip("the reference refuses this frame (no windows to take)")
    W, H = grid_of(ocomps, ow, oh)
    nc = len(samp)
    assert full.size == W * H * nc
    desc = J.image_desc(list(_to_j(ocomps)), qts, ow, oh, ct)
    for win in windows_for(W, H, seed=W * 31 + H):
        want = window_slice(full, W, H, nc, ct, win)
        rc, buf, ln = _decode(lib, desc, coefs, win, want.size)
        assert rc == 0, (win, rc)
        assert ln == want.size
        assert (buf[ln:] == 0x5A).all(), f"window {win}: the kernel wrote past the window's bytes"
        bad = np.nonzero(buf[:ln] != want)[0]
        assert bad.size == 0, (win, bad[:10], buf[bad[:10]], want[bad[:10]])


def _plan(lib, desc, win):
    geom = np.zeros(GEOM_WORDS, np.uint32)
    why = C.create_string_buffer(128)
    rc = lib.emu_window_plan(C.byref(desc), np.array(win, np.uint32).ctypes.data, geom.ctypes.data, GEOM_WORDS, why, 128)
    names = "scale ncomp hmax vmax mcu_w mcu_h align tx ry ox oy ex ey tiles_x bands".split()
    return rc, dict(zip(names, (int(v) for v in geom[:len(names)]))), why.value.decode()


PLAN_LAYOUTS = [([(2, 2), (1, 1), (1, 1)], "YCbCr"), ([(2, 1), (1, 1), (1, 1)], "YCbCr"), ([(1, 1)] * 3, "YCbCr"), ([(1, 1)], "Grayscale"),
                ([(4, 1), (1, 1), (1, 1)], "YCbCr"), ([(2, 2), (1, 1), (1, 1), (2, 2)], "YCCK")]


@pytest.mark.parametrize("layout", PLAN_LAYOUTS, ids=lambda l: f"{'_'.join(f'{h}{v}' for h, v in l[0])}-{l[1]}")
@pytest.mark.parametrize("scale", [8, 4, 2, 1])
def test_window_planner_tiles_cover_the_windows_mcu_rectangle(lib, layout, scale):
    """The launched tiles cover exactly the MCU rectangle of the window (its left edge rounded down to the tile alignment), and
    the rings of the tiles are clamped at the image's edges, never at the window's."""
    samp, ct = layout
    w_, h_ = 1921, 1083
    ocomps, _ = O.make_components(w_, h_, samp, dct_scale=scale)
    ow, oh = J.scaled_output_size(w_, h_, scale)
    qts = [np.ones(64, np.uint16) for _ in ocomps]
    desc = J.image_desc(list(_to_j(ocomps)), qts, ow, oh, ct)
    W, H = grid_of(ocomps, ow, oh)
    hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
    fancy = [len(samp) > 1 and (hmax // h, vmax // v) in ((2, 1), (1, 2), (2, 2)) for h, v in samp]
    for win in windows_for(W, H, seed=scale) + [(W // 4, H // 4, W // 2, H // 2)]:
        x, y, w, h = win
        rc, g, why = _plan(lib, desc, win)
        assert rc == 0, (win, why)
        mpx, mpy = hmax * scale, vmax * scale
        mx0, my0 = x // mpx, y // mpy
        mx1, my1 = min(-(-(x + w) // mpx), g["mcu_w"]), min(-(-(y + h) // mpy), g["mcu_h"])
        assert g["ox"] % g["align"] == 0 and g["ox"] <= mx0 < g["ox"] + g["align"], (win, g)
        assert (g["ox"] * mpx) % 8 == 0 and (g["tx"] * mpx) % 8 == 0
        assert (g["ex"], g["oy"], g["ey"]) == (mx1, my0, my1), (win, g)
        span_x, span_y = g["ex"] - g["ox"], g["ey"] - g["oy"]
        assert (g["tiles_x"] - 1) * g["tx"] < span_x <= g["tiles_x"] * g["tx"], (win, g)
        assert (g["bands"] - 1) * g["ry"] < span_y <= g["bands"] * g["ry"], (win, g)
        rect = np.zeros(4, np.int32)
        for band in range(g["bands"]):
            for tile in range(g["tiles_x"]):
                x0m, my = g["ox"] + tile * g["tx"], g["oy"] + band * g["ry"]
                te, re = min(g["tx"], g["ex"] - x0m), min(g["ry"], g["ey"] - my)
                for c, (hc, vc) in enumerate(samp):
                    assert lib.emu_window_tile_blocks(C.byref(desc), np.array(win, np.uint32).ctypes.data, tile, band, c, rect.ctypes.data) == 0
                    halo = 1 if fancy[c] else 0
                    bw, bh = ocomps[c].block_w, ocomps[c].block_h
                    want = (max(0, x0m * hc - halo), max(0, my * vc - halo), min(bw, (x0m + te) * hc + halo), min(bh, (my + re) * vc + halo))
                    assert tuple(int(v) for v in rect) == want, (win, tile, band, c)
        # a window edge inside the image: the ring reaches past it
        for c, (hc, vc) in enumerate(samp):
            if fancy[c] and 0 < g["ox"] and g["ex"] < g["mcu_w"]:
                lib.emu_window_tile_blocks(C.byref(desc), np.array(win, np.uint32).ctypes.data, 0, 0, c, rect.ctypes.data)
                assert rect[0] == g["ox"] * hc - 1


def test_window_planner_refuses_what_it_cannot_run(lib):
    ocomps, _ = O.make_components(64, 48, [(2, 2), (1, 1), (1, 1)], dct_scale=8)
    qts = [np.ones(64, np.uint16)] * 3
    desc = J.image_desc(list(_to_j(ocomps)), qts, 64, 48, "YCbCr")
    assert _plan(lib, desc, (0, 0, 64, 48))[0] == 0
    rc, _, why = _plan(lib, desc, (60, 0, 5, 1))
    assert rc == -1 and "outside" in why
    assert _plan(lib, desc, (0, 0, 0, 5))[0] == -1
    # a hand-made descriptor with components at different dct_scales (real streams give every component one: src/parser.rs:120-125)
    mixed = list(_to_j(ocomps))
    mixed[1].dct_scale = 4
    mixed[1].size_width, mixed[1].size_height = 16, 12
    desc2 = J.image_desc(mixed, qts, 64, 48, "YCbCr")
    rc, _, why = _plan(lib, desc2, (0, 0, 8, 8))
    assert rc != 0 and (rc > 0 or "dct_scale" in why)
    # a block grid update_component_sizes does not make (build_image_job accepts it: the planner names the reason)
    odd = list(_to_j(ocomps))
    odd[1].block_width += 1
    desc3 = J.image_desc(odd, qts, 64, 48, "YCbCr")
    rc, _, why = _plan(lib, desc3, (8, 8, 16, 16))
    assert rc == -1 and "block grid" in why
