"""CPU emulation of the placed resample kernels (csrc/placed_band.hpp, csrc/placed.hip) against the numpy statement of DESIGN.md §4.14.

tests/emu/emu_placement.cpp compiles the product's range tables, planner and kernel phases with g++ (the flags of tests/emu/Makefile) and
runs every workgroup of the launch grid lane by lane, the kernels' barriers as phase boundaries; the bytes must equal
tests/placement_ref.py's exactly, guard bytes behind the output must stay.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import placement_ref as P
import resample_ref as R
import rgb_ref as G
import tensor_ref as T

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
# the flags of tests/emu/Makefile
_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-DJPGPU_HOST_EMULATION"]
LDS = 32 * 1024  # RS_MAX_LDS
INFO = "rb job_bands cap_rows chunks lds_bytes bands pre fill_bands shared_bands vw vh shift".split()
FILL = (114, 7, 200, 33)


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("emu_placement")
    so = str(d / "libemuplacement.so")
    cmd = [os.environ.get("CXX", "g++"), *_FLAGS, "-shared", "-I", _EMU, "-include", os.path.join(_EMU, "hip_shim.hpp"), "-o", so,
           os.path.join(_EMU, "emu_placement.cpp")]
    subprocess.check_call(cmd)
    L = C.CDLL(so)
    u, i, p = C.c_uint32, C.c_int32, C.c_void_p
    L.emu_placed.argtypes = [p, u, u, u, u, u, u, u, u, i, i, p, p, u, u, p]
    L.emu_placed.restype = C.c_int
    L.emu_placed_tensor.argtypes = [p, u, u, u, u, u, u, u, u, i, i, p, p, u, u, u, p, p, u, u, p]
    L.emu_placed_tensor.restype = C.c_int
    L.emu_placed_range.argtypes = [u, u, u, u, p, p, u]
    L.emu_placed_range.restype = None
    L.emu_placed_fit.argtypes = [u, u, u, u, u, u, p]
    L.emu_placed_fit.restype = C.c_int
    return L


def _source(img, src_off):
    src = np.full(img.size + src_off + 8, 0xEE, np.uint8)
    src[src_off: src_off + img.size] = img.reshape(-1)
    return src


def run(lib, img, canvas, pl, fill=FILL, kind=0, src_off=0, lds_cap=LDS, rb_cap=64):
    """-> (out (ch, cw, channels), info dict).  The source starts `src_off` bytes into its buffer; a guard band behind the canvas must
    stay untouched."""
    H, W, nc = img.shape
    cw, ch = canvas
    onc = 3 if kind else nc
    src = _source(img, src_off)
    n = cw * ch * onc
    out = np.full(n + 64, 0x5A, np.uint8)
    info = np.zeros(16, np.uint32)
    f = np.asarray(fill, np.uint8)
    rc = lib.emu_placed(src.ctypes.data + src_off, W, H, nc, kind, cw, ch, pl[0], pl[1], pl[2], pl[3], f.ctypes.data, out.ctypes.data, lds_cap, rb_cap,
                        info.ctypes.data)
    assert rc == 0, rc
    assert (out[n:] == 0x5A).all(), "the kernel wrote past the canvas"
    return out[:n].reshape(ch, cw, onc), dict(zip(INFO, (int(v) for v in info[:len(INFO)])))


def run_tensor(lib, img, canvas, pl, fmt, flip, fill=FILL, kind=0, src_off=0, lds_cap=LDS, rb_cap=64):
    H, W, nc = img.shape
    cw, ch = canvas
    onc = 3 if kind else nc
    dtype, mean, std = fmt
    es = np.dtype(T.NP_DTYPE[dtype]).itemsize
    src = _source(img, src_off)
    n = cw * ch * onc * es
    raw = np.full(n + 64 + 16, 0x5A, np.uint8)
    o = (-raw.ctypes.data) % 16
    out = raw[o: o + n + 64]
    info = np.zeros(16, np.uint32)
    f = np.asarray(fill, np.uint8)
    mean, std = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    rc = lib.emu_placed_tensor(src.ctypes.data + src_off, W, H, nc, kind, cw, ch, pl[0], pl[1], pl[2], pl[3], f.ctypes.data, out.ctypes.data, 0, int(flip),
                               T.DTYPES.index(dtype) + 1, mean.ctypes.data, std.ctypes.data, lds_cap, rb_cap, info.ctypes.data)
    assert rc == 0, rc
    assert (out[n:] == 0x5A).all(), "the kernel wrote past the tensor"
    return out[:n].view(T.NP_DTYPE[dtype]).reshape(onc, ch, cw), dict(zip(INFO, (int(v) for v in info[:len(INFO)])))


def _img(rng, H, W, nc, kind="noise"):
    if kind == "extremes":
        return np.where(rng.random((H, W, nc)) < 0.5, 0, 255).astype(np.uint8)
    return rng.integers(0, 256, (H, W, nc), dtype=np.uint8)


def want_u8(img, canvas, pl, fill=FILL, kind=0):
    src = G.to_rgb(img) if kind else img
    return P.place(src, canvas[0], canvas[1], pl, fill)


def test_range_tables_are_slices_of_the_numpy_tables(lib):
    rng = np.random.default_rng(3)
    for in_size, out_size in [(1, 1), (1, 65535), (65535, 1), (1080, 455), (375, 256), (997, 13), (13, 997), (3, 7)]:
        wb, wk = R.coefficients(in_size, out_size)
        ks = wk.shape[1]
        ranges = [(0, out_size), (0, 1), (out_size - 1, 1)] + [tuple(sorted(int(v) for v in rng.integers(0, out_size + 1, 2))) for _ in range(4)]
        for first, end in ranges:
            count = (end - first) if end > first else 0
            count = min(count, 4096) if out_size > 4096 else count
            if count == 0:
                continue
            b, k = np.full((count, 2), -1, np.int32), np.full((count, ks), -1, np.int32)
            lib.emu_placed_range(in_size, out_size, first, count, b.ctypes.data, k.ctypes.data, ks)
            assert np.array_equal(b, wb[first:first + count]) and np.array_equal(k, wk[first:first + count]), (in_size, out_size, first, count)


# (H, W, canvas, placement): crop on both axes with odd offsets, pad on both, crop in x with pad in y, up-scaling x3, the evaluation
# transform and the letterbox of small sizes, the identity, a canvas row that is no multiple of four bytes
CASES = [(75, 100, (56, 56), (85, 64, -15, -3)), (17, 9, (37, 53), (27, 51, 5, 1)), (34, 50, (37, 53), (61, 20, -11, 17)), (34, 50, (64, 64), (150, 102, -43, -19)),
         (97, 161, (224, 224), (224, 135, 0, 44)), (50, 34, (7, 9), (21, 30, -7, -11)), (50, 34, (2048, 3), (102, 150, 1000, -70)), (31, 33, (33, 31), (33, 31, 0, 0)),
         (40, 40, (20, 24), (9, 9, 11, 15)), (12, 200, (224, 224), (224, 13, 0, 105))]


@pytest.mark.parametrize("nc", [1, 3, 4])
@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[1]}x{c[0]}-{c[2][0]}x{c[2][1]}-{'_'.join(str(v) for v in c[3])}")
def test_placed_kernel_logic_matches_the_numpy_statement(lib, case, nc):
    H, W, canvas, pl = case
    rng = np.random.default_rng(H * 7 + W * 131 + nc * 1009 + pl[0])
    for kind in ("noise", "extremes"):
        img = _img(rng, H, W, nc, kind)
        want = want_u8(img, canvas, pl)
        for src_off in (0, 1, 3):
            got, info = run(lib, img, canvas, pl, src_off=src_off)
            assert info["chunks"] == 1 and info["lds_bytes"] <= LDS, info
            assert np.array_equal(got, want), (case, nc, kind, src_off, info, np.argwhere(got != want)[:5].tolist())


@pytest.mark.parametrize("nc", [1, 3, 4])
def test_bands_without_a_visible_row_and_bands_that_share_dwords(lib, nc):
    """Mostly padding — canvas (16, 200), eight visible rows at y = 150: the bands above and below write fill and read nothing (LDS is
    garbage there).  Bands of 1, 2, 3, 5 and 7 rows over a canvas row of no multiple of four bytes: first and last dwords are shared,
    every band stores its own bytes only."""
    rng = np.random.default_rng(nc)
    img = _img(rng, 97, 161, nc)
    got, info = run(lib, img, (16, 200), (5, 8, 6, 150))
    assert info["vh"] == 8 and info["rb"] == 8 and info["fill_bands"] == info["bands"] - 1 >= 24, info
    assert np.array_equal(got, want_u8(img, (16, 200), (5, 8, 6, 150)))
    seen_shared = 0
    for (H, W, canvas, pl) in [(61, 47, (13, 17), (21, 9, -3, 5)), (40, 40, (21, 40), (30, 50, 2, -7)), (9, 100, (33, 23), (20, 20, 14, 1)), (233, 10, (7, 11), (9, 5, -1, 3))]:
        img = _img(rng, H, W, nc)
        want = want_u8(img, canvas, pl)
        for rb_cap in (1, 2, 3, 5, 7):
            got, info = run(lib, img, canvas, pl, src_off=1, rb_cap=rb_cap)
            assert info["rb"] <= rb_cap and info["bands"] >= info["job_bands"] + info["pre"], info
            seen_shared += info["shared_bands"]
            assert np.array_equal(got, want), (H, W, canvas, pl, rb_cap, info)
    if nc != 4:
        assert seen_shared > 0


@pytest.mark.parametrize("nc", [1, 3, 4])
def test_chunked_vertical_path_with_a_placement(lib, nc):
    """An LDS budget of a few rows, and the real budget with a 24 x 1100 source squeezed to one row at (1, 3) of a 7 x 7 canvas: an
    output row's support takes several chunks; rows of fill lie above and below it."""
    rng = np.random.default_rng(40 + nc)
    for (H, W, canvas, pl) in [(300, 20, (9, 6), (7, 2, 1, 3)), (64, 64, (64, 9), (80, 5, -9, 2)), (1100, 24, (7, 7), (2, 1, 1, 3)), (97, 400, (300, 5), (300, 3, 0, 1)),
                               (1200, 16, (2048, 2), (2500, 1, -200, 1))]:
        img = _img(rng, H, W, nc)
        want = want_u8(img, canvas, pl)
        for rows in (1, 2, 5):
            vw = min(canvas[0], pl[2] + pl[0]) - max(0, pl[2])
            pitch = (((max(0, pl[2]) * nc) & 15) + vw * nc + 15) & ~15
            got, info = run(lib, img, canvas, pl, src_off=3, lds_cap=pitch * rows + 3)
            assert info["cap_rows"] == min(rows, H, LDS // pitch), info
            assert info["chunks"] > 1 and info["rb"] == 1, info
            assert np.array_equal(got, want), (H, W, canvas, pl, nc, rows, info)
    img = _img(rng, 1100, 24, nc)
    got, info = run(lib, img, (7, 7), (2, 1, 1, 3), lds_cap=64)  # (four rows of 16 bytes)
    assert info["chunks"] > 1 and info["fill_bands"] == 6, info
    assert np.array_equal(got, want_u8(img, (7, 7), (2, 1, 1, 3)))


@pytest.mark.parametrize("nc", [1, 3, 4])
def test_one_visible_pixel_at_every_corner(lib, nc):
    rng = np.random.default_rng(70 + nc)
    img = _img(rng, 97, 131, nc)
    for canvas in [(3, 3), (224, 224), (37, 53), (2048, 3)]:
        cw, ch = canvas
        for pl in [(61, 45, -60, -44), (61, 45, cw - 1, -44), (61, 45, -60, ch - 1), (61, 45, cw - 1, ch - 1)]:
            got, info = run(lib, img, canvas, pl)
            assert info["vw"] == 1 and info["vh"] == 1, info
            want = want_u8(img, canvas, pl)
            assert np.array_equal(got, want), (canvas, pl, info)
            assert (got != np.asarray(FILL[:nc], np.uint8)).any(axis=2).sum() <= 1


def test_rgb_sources_with_a_placement(lib):
    """The converting horizontal passes (gray, CMYK) under a placement; the fill is in RGB order."""
    rng = np.random.default_rng(12)
    for nc in (1, 4):
        for (H, W, canvas, pl) in [(34, 50, (37, 53), (20, 30, 9, 11)), (75, 100, (56, 56), (85, 64, -15, -3)), (300, 20, (9, 6), (7, 2, 1, 3))]:
            img = _img(rng, H, W, nc)
            got, info = run(lib, img, canvas, pl, kind=nc, lds_cap=LDS if H < 300 else 64)
            assert np.array_equal(got, want_u8(img, canvas, pl, kind=nc)), (nc, H, W, canvas, pl, info)


FMTS = [("float32",) + T.IMAGENET, ("bfloat16",) + T.CLIP, ("float16",) + T.HALF]


@pytest.mark.parametrize("fmt", FMTS, ids=lambda f: f[0])
@pytest.mark.parametrize("nc", [1, 3, 4])
def test_placed_tensor_kernel_matches_the_numpy_statement(lib, nc, fmt):
    """Canvases of four-pixel items (224 x 224, 64 x 8) and of element-wise items (37 x 53, 7 x 9); flips mirror the finished canvas; a
    filled element is T[c][fill[c]]."""
    rng = np.random.default_rng(nc * 31 + len(fmt[0]))
    tab = T.table(fmt, nc)
    for (H, W, canvas, pl) in [(75, 100, (224, 224), (85, 64, 70, 101)), (75, 100, (64, 8), (85, 64, -15, -3)), (34, 50, (37, 53), (61, 20, -11, 17)),
                               (17, 9, (37, 53), (27, 51, 5, 1)), (50, 34, (7, 9), (21, 30, -7, -11)), (97, 131, (224, 224), (61, 45, 223, 223)),
                               (34, 50, (224, 224), (150, 102, 37, 61)), (34, 50, (224, 224), (150, 102, 38, -3)), (34, 50, (224, 224), (250, 300, -13, -3))]:
        img = _img(rng, H, W, nc)
        u8 = want_u8(img, canvas, pl)
        for flip in (False, True):
            got, info = run_tensor(lib, img, canvas, pl, fmt, flip, src_off=2)
            want = T.to_tensor(u8, tab, flip)
            assert np.array_equal(T.bits(got), T.bits(want)), (nc, fmt[0], H, W, canvas, pl, flip, info, np.argwhere(T.bits(got) != T.bits(want))[:5].tolist())


def test_placed_tensor_chunked_path_and_bands_of_fill(lib):
    rng = np.random.default_rng(5)
    fmt = FMTS[0]
    for nc in (1, 3):
        tab = T.table(fmt, nc)
        for (H, W, canvas, pl, cap) in [(1100, 24, (8, 8), (2, 1, 1, 3), 64), (1100, 24, (7, 7), (2, 1, 1, 3), 64), (300, 20, (1040, 4), (1100, 2, -30, 1), 2 * 1040 * 3 + 64),
                                        (97, 161, (16, 200), (5, 8, 6, 150), LDS)]:
            img = _img(rng, H, W, nc)
            u8 = want_u8(img, canvas, pl)
            for flip in (False, True):
                got, info = run_tensor(lib, img, canvas, pl, fmt, flip, lds_cap=cap)
                assert info["fill_bands"] > 0 and (cap == LDS or info["chunks"] > 1), info
                assert np.array_equal(T.bits(got), T.bits(T.to_tensor(u8, tab, flip))), (nc, H, W, canvas, pl, flip, info)


def test_fit_rules_in_the_emulation_build(lib):
    out = np.zeros(4, np.int32)
    assert lib.emu_placed_fit(1, 256, 500, 375, 224, 224, out.ctypes.data) == 0 and tuple(out) == (341, 256, -58, -16)
    assert lib.emu_placed_fit(2, 0, 1920, 1080, 640, 640, out.ctypes.data) == 0 and tuple(out) == (640, 360, 0, 140)
    assert lib.emu_placed_fit(1, 256, 8, 4000, 224, 224, out.ctypes.data) == -1
    assert lib.emu_placed_fit(3, 0, 8, 8, 8, 8, out.ctypes.data) == -1
