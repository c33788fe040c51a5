"""CPU emulation of the band kernels (csrc/resample_band.hpp, tensor_band.hpp, placed_band.hpp) under the filters of DESIGN.md §4.15.

tests/emu/emu_filters.cpp compiles the product's filtered tables, planners and kernel phases with g++ (the flags of tests/emu/Makefile)
and runs every workgroup of the launch grid lane by lane, the kernels' barriers as phase boundaries; the bytes must equal
tests/filter_ref.py's exactly.  The kernels are the ones BILINEAR runs: what is new to them is wider tables and negative weights, so
the sources are 0 / 255 block patterns on which both passes leave 0..255 (asserted).  Then the run kernels (runs of bands): every
workgroup, the move of the kept rows in its read and write phases, and which plans take the route.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import filter_ref as F
import rgb_ref
import tensor_ref as T

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
# the flags of tests/emu/Makefile
_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-DJPGPU_HOST_EMULATION"]
LDS = 32 * 1024  # RS_MAX_LDS
FILTERS = ["bilinear", "box", "hamming", "bicubic", "lanczos"]
NEW = FILTERS[1:]
ONE = 255 << 22
INFO = "rb bands cap_rows chunks lds_bytes launch_bands hks vks hneg vneg".split()


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("emu_filters")
    so = str(d / "libemufilters.so")
    cmd = [os.environ.get("CXX", "g++"), *_FLAGS, "-shared", "-I", _EMU, "-include", os.path.join(_EMU, "hip_shim.hpp"), "-o", so,
           os.path.join(_EMU, "emu_filters.cpp")]
    subprocess.check_call(cmd)
    L = C.CDLL(so)
    L.emu_filter_u8.argtypes = [C.c_void_p] * 5
    L.emu_filter_u8.restype = C.c_int
    L.emu_filter_tensor.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    L.emu_filter_tensor.restype = C.c_int
    L.emu_filter_ksize.argtypes = [C.c_uint32] * 3
    L.emu_filter_ksize.restype = C.c_uint32
    L.emu_filter_ksize_old.argtypes = [C.c_uint32] * 2
    L.emu_filter_ksize_old.restype = C.c_uint32
    L.emu_filter_tables.argtypes = [C.c_uint32] * 5 + [C.c_void_p, C.c_void_p, C.c_uint32]
    L.emu_filter_tables_old.argtypes = [C.c_uint32] * 4 + [C.c_void_p, C.c_void_p, C.c_uint32]
    return L


def blocks(seed, H, W, nc, sy=2, sx=None):
    """0 / 255 blocks of sy x sx pixels: the images on which negative lobes leave 0..255 (blocks about as large as the filter's
    support in source pixels overshoot most)."""
    sx = sy if sx is None else sx
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 2, ((H + sy - 1) // sy, (W + sx - 1) // sx, nc), dtype=np.uint8) * np.uint8(255)
    return np.ascontiguousarray(a.repeat(sy, axis=0).repeat(sx, axis=1)[:H, :W])


def _geom(f, img, kind, ow, oh, place, lds_cap, rb_cap):
    H, W, nc = img.shape
    rw, rh, x, y = place if place is not None else (ow, oh, 0, 0)
    return np.array([f, W, H, nc, kind, ow, oh, 0 if place is None else 1, rw, rh, x & 0xffffffff, y & 0xffffffff, lds_cap, rb_cap], np.uint32)


def _src(img, src_off):
    src = np.full(img.size + src_off + 8, 0xEE, np.uint8)
    src[src_off: src_off + img.size] = img.reshape(-1)
    return src


def run(lib, f, img, ow, oh, kind=0, place=None, fill=(0, 0, 0, 0), src_off=0, lds_cap=LDS, rb_cap=64):
    """-> (out (oh, ow, channels), info).  The source starts `src_off` bytes into its buffer (window rows start anywhere; CMYK sources
    are dword-aligned as the batch lays them); a guard band behind the output must stay untouched."""
    onc = 3 if kind else img.shape[2]
    src = _src(img, src_off)
    n = ow * oh * onc
    out = np.full(n + 64, 0x5A, np.uint8)
    info = np.zeros(16, np.uint32)
    g = _geom(f, img, kind, ow, oh, place, lds_cap, rb_cap)
    fl = np.array(fill, np.uint8)
    rc = lib.emu_filter_u8(g.ctypes.data, src.ctypes.data + src_off, fl.ctypes.data, out.ctypes.data, info.ctypes.data)
    assert rc == 0, rc
    assert (out[n:] == 0x5A).all(), "the kernel wrote past the image's bytes"
    return out[:n].reshape(oh, ow, onc), dict(zip(INFO, (int(v) for v in info[:10])))


def run_tensor(lib, f, img, ow, oh, fmt, flip, kind=0, place=None, fill=(0, 0, 0, 0), src_off=0, lds_cap=LDS, rb_cap=64):
    onc = 3 if kind else img.shape[2]
    dtype, mean, std = fmt
    es = 4 if dtype == "float32" else 2
    src = _src(img, src_off)
    n = ow * oh * onc * es
    raw = np.full(n + 64 + 16, 0x5A, np.uint8)
    off = (-raw.ctypes.data) & 15
    out = raw[off: off + n + 64]
    info = np.zeros(16, np.uint32)
    g = _geom(f, img, kind, ow, oh, place, lds_cap, rb_cap)
    fl = np.array(fill, np.uint8)
    m, s = np.array(mean, np.float32), np.array(std, np.float32)
    rc = lib.emu_filter_tensor(g.ctypes.data, src.ctypes.data + src_off, fl.ctypes.data, out.ctypes.data, 1 if flip else 0, T.DTYPES.index(dtype) + 1,
                               m.ctypes.data, s.ctypes.data, info.ctypes.data)
    assert rc == 0, rc
    assert (out[n:] == 0x5A).all(), "the kernel wrote past the image's bytes"
    return out[:n].view(T.NP_DTYPE[dtype]).reshape(onc, oh, ow), dict(zip(INFO, (int(v) for v in info[:10])))


def want_u8(f, img, ow, oh, kind=0, place=None, fill=(0, 0, 0, 0), sums=None):
    src = rgb_ref.to_rgb(img) if kind else img
    if place is None:
        return F.resize(src, ow, oh, f, sums=sums)
    return F.placed(src, *place, ow, oh, fill, f)


def clamps_at_both_ends(sums):
    """The unclamped sums of the horizontal AND of the vertical pass leave 0..255 on both sides."""
    return len(sums) == 2 and all(lo < 0 and hi >= ONE + (1 << 22) for lo, hi in sums)


def test_inline_functions_that_were_there_equal_filter_0(lib):
    for in_size, out_size in [(1, 1), (1, 2048), (65535, 1), (1080, 224), (224, 224), (997, 13), (13, 997), (540, 224), (3, 7), (2039, 251)]:
        ks = lib.emu_filter_ksize(0, in_size, out_size)
        assert ks == lib.emu_filter_ksize_old(in_size, out_size) == F.ksize_of(in_size, out_size)
        for first, count in [(0, out_size), (out_size // 2, out_size - out_size // 2)]:
            b, k = np.full((count, 2), -1, np.int32), np.full((count, ks), -1, np.int32)
            ob, ok = b.copy(), k.copy()
            lib.emu_filter_tables(0, in_size, out_size, first, count, b.ctypes.data, k.ctypes.data, ks)
            lib.emu_filter_tables_old(in_size, out_size, first, count, ob.ctypes.data, ok.ctypes.data, ks)
            assert np.array_equal(b, ob) and np.array_equal(k, ok), (in_size, out_size, first)


@pytest.mark.parametrize("name", FILTERS)
def test_inline_tables_are_the_statements(lib, name):
    f = F.NAMES[name]
    for in_size, out_size in [(1, 1), (1, 300), (4093, 1), (1080, 224), (224, 224), (997, 13), (13, 997), (375, 224), (3, 7), (2160, 224)]:
        ks = lib.emu_filter_ksize(f, in_size, out_size)
        wb, wk = F.coefficients_range(in_size, out_size, 0, out_size, f)
        assert ks == wk.shape[1]
        b, k = np.full((out_size, 2), -1, np.int32), np.full((out_size, ks), -1, np.int32)
        lib.emu_filter_tables(f, in_size, out_size, 0, out_size, b.ctypes.data, k.ctypes.data, ks)
        assert np.array_equal(b, wb) and np.array_equal(k, wk), (in_size, out_size)


# the shapes of tests/test_gpu_filters.py: (H, W, ow, oh)
WINDOW = (61, 97, 37, 53)  # a 97 x 61 image to (37, 53)
UP = (7, 9, 64, 48)        # a 9 x 7 window up to 64 x 48: overshoot at scale < 1
TALL = (400, 64, 24, 40)   # bands whose source rows overlap three to six times under the wide filters
BLOCK = {WINDOW: (8, 8), UP: (2, 2), TALL: (40, 8)}  # the block sizes on which both passes overshoot at these scales


@pytest.mark.parametrize("nc,kind", [(3, 0), (1, 0), (4, 0), (1, 1), (4, 4)], ids=["ycc", "gray", "cmyk", "gray-rgb", "cmyk-rgb"])
@pytest.mark.parametrize("name", NEW)
def test_band_kernel_under_every_filter(lib, name, nc, kind):
    f = F.NAMES[name]
    for shape in (WINDOW, UP, TALL):
        H, W, ow, oh = shape
        img = blocks(H + W + nc, H, W, nc, *BLOCK[shape])
        sums = []
        want = want_u8(f, img, ow, oh, kind, sums=sums)
        if name in ("bicubic", "lanczos"):
            assert clamps_at_both_ends(sums), sums  # (else the clamps are not tested)
        for src_off in ((0,) if nc == 4 else (0, 1, 3)):  # (window rows at odd byte offsets)
            got, info = run(lib, f, img, ow, oh, kind, src_off=src_off)
            assert info["chunks"] == 1 and info["lds_bytes"] <= LDS, info
            assert info["hneg"] == info["vneg"] == (name in ("bicubic", "lanczos")), info
            assert np.array_equal(got, want), (name, shape, nc, kind, src_off, info, np.argwhere(got != want)[:5].tolist())


@pytest.mark.parametrize("name", FILTERS)
def test_output_size_equal_to_the_window_is_the_window(lib, name):
    f = F.NAMES[name]
    for nc in (1, 3, 4):
        img = blocks(9 + nc, 37, 53, nc, 1)
        got, _info = run(lib, f, img, 53, 37, src_off=0 if nc == 4 else 1)
        assert np.array_equal(got, img)


@pytest.mark.parametrize("name", ["bicubic", "lanczos"])
def test_chunked_path_with_negative_partial_sums(lib, name):
    """A 16 x 1200 image to (16, 1), (16, 2) and (16, 3): an output row's support takes several chunks.  With ONE output row the
    filter's argument stays inside (-0.5, 0.5) and every weight is positive; with two or three rows the supports reach the negative
    lobes, and a chunk that lies wholly inside one leaves a negative partial sum in the registers (asserted on the tables)."""
    f = F.NAMES[name]
    for nc in (1, 3, 4):
        img = blocks(70 + nc, 1200, 16, nc, 150, 3)
        pitch = (16 * nc + 3) & ~3
        for oh in (1, 2, 3):
            want = F.resize(img, 16, oh, f)
            vb, vk = F.coefficients(1200, oh, f)
            assert (vk < 0).any() == (oh > 1)
            for rows in (37, 200, LDS // pitch):
                got, info = run(lib, f, img, 16, oh, lds_cap=pitch * rows)
                assert info["cap_rows"] == min(rows, 1200) and info["chunks"] == -(-int(vb[:, 1].max()) // info["cap_rows"]), info
                assert info["chunks"] > 1 or (nc == 1 and rows > 200), info  # (at the real budget only 16-byte rows fit whole)
                assert info["rb"] == 1 or info["chunks"] == 1, info
                if oh > 1 and rows == 37:  # (some chunk lies wholly inside a negative lobe)
                    k = vk[0, : vb[0, 1]]
                    assert any((k[c: c + rows] <= 0).all() and (k[c: c + rows] < 0).any() for c in range(0, len(k), rows))
                assert np.array_equal(got, want), (name, nc, oh, rows, info)
    # a random image as well: the sums far from the clamps
    img = np.random.default_rng(3).integers(0, 256, (1200, 16, 3), dtype=np.uint8)
    got, info = run(lib, f, img, 16, 3, lds_cap=48 * 50)
    assert info["chunks"] > 1 and np.array_equal(got, F.resize(img, 16, 3, f))


@pytest.mark.parametrize("name", NEW)
def test_a_plan_with_one_row_per_band_in_one_chunk(lib, name):
    """rb == 1 because no two output rows' source rows fit in LDS together, while one row's still do: a band of one row on the
    one-chunk path (group_columns narrows nothing there)."""
    f = F.NAMES[name]
    H, W, ow, oh, nc = 300, 40, 33, 10, 3
    img = blocks(5, H, W, nc, 3)
    vb, _ = F.coefficients(H, oh, f)
    pitch = (ow * nc + 3) & ~3
    rows = int(vb[:, 1].max())
    got, info = run(lib, f, img, ow, oh, src_off=1, lds_cap=pitch * rows)
    assert info["rb"] == 1 and info["chunks"] == 1 and info["bands"] == oh and info["cap_rows"] == rows, info
    assert np.array_equal(got, F.resize(img, ow, oh, f))


@pytest.mark.parametrize("fmt", [("float32",) + T.IMAGENET, ("bfloat16",) + T.CLIP, ("float16",) + T.HALF], ids=lambda f: f[0])
@pytest.mark.parametrize("name", NEW)
def test_tensor_kernel_under_every_filter(lib, name, fmt):
    f = F.NAMES[name]
    for (H, W, ow, oh), nc, kind in [(WINDOW, 3, 0), (TALL, 1, 1), (UP, 4, 4), (WINDOW, 1, 0)]:
        img = blocks(H + nc, H, W, nc, *BLOCK[(H, W, ow, oh)])
        onc = 3 if kind else nc
        u8 = want_u8(f, img, ow, oh, kind)
        for flip in (False, True):
            got, info = run_tensor(lib, f, img, ow, oh, fmt, flip, kind, src_off=0 if nc == 4 else 3)
            want = T.to_tensor(u8, T.table(fmt, onc), flip)
            assert np.array_equal(T.bits(got), T.bits(want)), (name, fmt[0], nc, kind, flip, info)


@pytest.mark.parametrize("name", ["bicubic", "lanczos"])
def test_tensor_kernel_chunked(lib, name):
    f = F.NAMES[name]
    fmt = ("float32",) + T.IMAGENET
    img = blocks(8, 1200, 16, 3, 150, 3)
    got, info = run_tensor(lib, f, img, 16, 3, fmt, True, lds_cap=48 * 37)
    assert info["chunks"] > 1, info
    want = T.to_tensor(F.resize(img, 16, 3, f), T.table(fmt, 3), True)
    assert np.array_equal(T.bits(got), T.bits(want))


# (H, W, nc, kind, (rw, rh, x, y), ow, oh, fill): a letterbox, a shorter-side crop partly outside the canvas (range tables with
# first > 0 on one axis, fill on the other), a crop on both axes, an up-scaled source cropped at every edge
PLACEMENTS = [(61, 97, 3, 0, (48, 30, 0, 9), 48, 48, (114, 114, 114, 0)), (61, 97, 3, 0, (76, 48, -14, 0), 48, 48, (0, 0, 0, 0)),
              (400, 64, 1, 1, (24, 150, 5, -60), 37, 53, (9, 8, 7, 0)), (61, 97, 4, 4, (60, 40, -21, 30), 37, 53, (1, 2, 3, 4)),
              (7, 9, 1, 0, (64, 48, -10, -5), 37, 41, (200, 0, 0, 0))]


@pytest.mark.parametrize("name", NEW)
def test_placed_kernels_under_every_filter(lib, name):
    f = F.NAMES[name]
    fmt = ("bfloat16",) + T.CLIP
    for H, W, nc, kind, place, ow, oh, fill in PLACEMENTS:
        img = blocks(H * 3 + nc, H, W, nc, 40 if H == 400 else 8 if H == 61 else 2, 2 if H == 7 else 8)
        onc = 3 if kind else nc
        want = want_u8(f, img, ow, oh, kind, place, fill)
        got, info = run(lib, f, img, ow, oh, kind, place, fill, src_off=0 if nc == 4 else 1)
        assert np.array_equal(got, want), (name, place, info, np.argwhere(got != want)[:5].tolist())
        for flip in (False, True):
            gt, info = run_tensor(lib, f, img, ow, oh, fmt, flip, kind, place, fill, src_off=0 if nc == 4 else 1)
            assert np.array_equal(T.bits(gt), T.bits(T.to_tensor(want, T.table(fmt, onc), flip))), (name, place, flip, info)
    # the placed kernels' chunked path: a tall source squeezed into a few visible rows
    img = blocks(77, 1200, 16, 3, 3)
    place, fill = (16, 3, 4, -1), (5, 6, 7, 0)
    got, info = run(lib, f, img, 24, 4, 0, place, fill, lds_cap=48 * 29)
    assert info["chunks"] > 1, info
    assert np.array_equal(got, F.placed(img, *place, 24, 4, fill, f))


# ---- runs of bands (resample_run_kernel / resample_tensor_run_kernel) -------------------------------------------------------------------
RUN_INFO = "rb bands cap_rows bpr lds_bytes runs last_run moved reused read passed".split()


def _run_lib(lib):
    lib.emu_filter_run_u8.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emu_filter_run_u8.restype = C.c_int
    lib.emu_filter_run_tensor.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.emu_filter_run_tensor.restype = C.c_int
    return lib


def run_runs(lib, f, img, ow, oh, bpr, kind=0, src_off=0, phases=1, lds_cap=LDS, rb_cap=64, fmt=None, flip=False):
    """The run kernels: -> (rc, out, info).  fmt: the tensor kernel."""
    _run_lib(lib)
    onc = 3 if kind else img.shape[2]
    es = 1 if fmt is None else (4 if fmt[0] == "float32" else 2)
    src = _src(img, src_off)
    n = ow * oh * onc * es
    raw = np.full(n + 64 + 16, 0x5A, np.uint8)
    off = (-raw.ctypes.data) & 15
    out = raw[off: off + n + 64]
    info = np.zeros(16, np.uint32)
    g = _geom(f, img, kind, ow, oh, None, lds_cap, rb_cap)
    if fmt is None:
        rc = lib.emu_filter_run_u8(g.ctypes.data, bpr, phases, src.ctypes.data + src_off, out.ctypes.data, info.ctypes.data)
    else:
        m, s = np.array(fmt[1], np.float32), np.array(fmt[2], np.float32)
        rc = lib.emu_filter_run_tensor(g.ctypes.data, bpr, phases, src.ctypes.data + src_off, out.ctypes.data, 1 if flip else 0, T.DTYPES.index(fmt[0]) + 1,
                                       m.ctypes.data, s.ctypes.data, info.ctypes.data)
    if rc:
        return rc, None, None
    assert (out[n:] == 0x5A).all(), "the kernel wrote past the image's bytes"
    got = out[:n].reshape(oh, ow, onc) if fmt is None else out[:n].view(T.NP_DTYPE[fmt[0]]).reshape(onc, oh, ow)
    return 0, got, dict(zip(RUN_INFO, (int(v) for v in info[:11])))


# (H, W, ow, oh, nc): plans of many bands whose source rows overlap — a 64 x 1080 source to (224, 225) is the shape of the GPU test
RUNS = [(1080, 64, 224, 225, 3), (2000, 96, 24, 200, 3), (700, 50, 60, 37, 4), (375, 61, 37, 224, 1)]


@pytest.mark.parametrize("bpr", [2, 4, 8])
@pytest.mark.parametrize("name", ["bicubic", "lanczos"])
def test_run_kernel_every_workgroup(lib, name, bpr):
    f = F.NAMES[name]
    for H, W, ow, oh, nc in RUNS:
        for kind in ((0, 1) if nc == 1 else (0, 4) if nc == 4 else (0,)):
            img = blocks(H + bpr, H, W, nc, max(2, H // oh * 3), 8)
            want = want_u8(f, img, ow, oh, kind)
            rc, got, info = run_runs(lib, f, img, ow, oh, bpr, kind, src_off=0 if nc == 4 else 1)
            assert rc == 0 and info["bpr"] == bpr and info["runs"] == -(-info["bands"] // bpr) and info["lds_bytes"] <= LDS, info
            assert info["reused"] > 0 and info["passed"] > info["read"], info  # (rows did skip the horizontal pass)
            assert np.array_equal(got, want), (name, bpr, (H, W, ow, oh, nc), kind, info, np.argwhere(got != want)[:5].tolist())
            band, _i = run(lib, f, img, ow, oh, kind, src_off=0 if nc == 4 else 1)
            assert np.array_equal(band, got)  # (and the band kernels give the same bytes)
            # short bands: the kept rows outnumber the rows they move by — the move overlaps itself
            rc, got, info = run_runs(lib, f, img, ow, oh, bpr, kind, src_off=0 if nc == 4 else 1, rb_cap=1 + bpr % 3)
            assert rc == 0 and info["rb"] <= 1 + bpr % 3 and np.array_equal(got, want), (name, bpr, (H, W, ow, oh, nc), kind, info)


def test_the_gpu_tests_run_shape_has_the_plan_it_needs(lib):
    """64 x 1080 to (224, 225): at least two runs, at least three bands in a run, a shorter last run — for the bpr the rule picks.  (A
    64 x 400 source to (24, 40) plans ONE band: 400 rows of 72 bytes fit in LDS.)"""
    for name in ("bicubic", "lanczos"):
        img = blocks(3, 1080, 64, 3, 15, 8)
        rc, got, info = run_runs(lib, F.NAMES[name], img, 224, 225, 0)
        assert rc == 0, (name, rc)  # (the rule takes the route for this plan)
        assert info["runs"] >= 2 and info["bpr"] >= 3 and 0 < info["last_run"] < info["bpr"], info
        assert info["moved"] > 0, info
        assert np.array_equal(got, F.resize(img, 224, 225, F.NAMES[name]))


@pytest.mark.parametrize("fmt", [("float32",) + T.IMAGENET, ("bfloat16",) + T.CLIP], ids=lambda f: f[0])
def test_tensor_run_kernel(lib, fmt):
    for name in ("bicubic", "lanczos"):
        f = F.NAMES[name]
        for (H, W, ow, oh, nc), kind in ((RUNS[0], 0), (RUNS[3], 1), (RUNS[2], 4), (RUNS[1], 0)):
            img = blocks(H, H, W, nc, max(2, H // oh * 3), 8)
            onc = 3 if kind else nc
            want = T.to_tensor(want_u8(f, img, ow, oh, kind), T.table(fmt, onc), True)
            rc, got, info = run_runs(lib, f, img, ow, oh, 4, kind, src_off=0 if nc == 4 else 3, fmt=fmt, flip=True)
            assert rc == 0 and info["reused"] > 0, info
            assert np.array_equal(T.bits(got), T.bits(want)), (name, fmt[0], (H, W, ow, oh, nc), kind, info)


def test_a_move_without_the_read_and_write_phases_fails_here(lib):
    """The move goes toward lower addresses and overlaps itself.  With every lane reading and writing in turn (phases = 0) a lane's
    write lands on a dword a later lane has yet to read: this emulation, which runs lanes one after another, must see that."""
    f = F.NAMES["lanczos"]
    H, W, ow, oh, nc = RUNS[0]
    img = blocks(11, H, W, nc, 15, 8)
    want = F.resize(img, ow, oh, f)
    # bands of one output row: a band keeps ~24 rows and moves them down by 4 or 5 — less than it keeps, and less than a slab
    rc, good, info = run_runs(lib, f, img, ow, oh, 4, phases=1, rb_cap=1)
    assert rc == 0 and info["rb"] == 1 and info["reused"] > 3 * info["read"] and np.array_equal(good, want), info
    rc, bad, _info = run_runs(lib, f, img, ow, oh, 4, phases=0, rb_cap=1)
    assert rc == 0 and not np.array_equal(bad, want)


def test_which_plans_take_the_route(lib):
    """BILINEAR, BOX and HAMMING never; BICUBIC and LANCZOS above the redundancy the rule sets; chunked plans and single bands never."""
    img = blocks(1, 1080, 64, 3, 15, 8)
    for name in ("bilinear", "box", "hamming"):
        for bpr in (0, 2, 4, 8):
            assert run_runs(lib, F.NAMES[name], img, 224, 225, bpr)[0] == -4, name
    for name in ("bicubic", "lanczos"):
        f = F.NAMES[name]
        assert run_runs(lib, f, img, 224, 225, 1)[0] == -4                      # (the knob's "never")
        assert run_runs(lib, f, img[:400], 24, 40, 0)[0] == -4                  # (one band: 400 rows of 72 bytes fit in LDS)
        assert run_runs(lib, f, img[:1000], 16, 3, 4, lds_cap=48 * 37)[0] == -4  # (chunked bands keep their bands)
        small = blocks(2, 375, 500, 3, 8)
        rc, _g, info = run_runs(lib, f, small, 224, 224, 4)
        assert rc == 0 and info["passed"] * 100 <= info["read"] * 130, info     # (forced: a plan the rule leaves alone ...)
        assert run_runs(lib, f, small, 224, 224, 0)[0] == -4                    # (... because its redundancy is low)
