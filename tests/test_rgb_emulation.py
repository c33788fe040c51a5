"""CPU emulation of the RGB-output kernels (csrc/resample_band.hpp RBand::hpass_walk / hpass_cmyk behind resample_band_rgb_kernel and
resample_tensor_rgb_kernel) against the numpy statement of DESIGN.md §4.12: convert, then resample.

tests/emu/emu_rgb.cpp compiles the product's tables, planner and kernel phases with g++ (the flags of tests/emu/Makefile) and runs every
workgroup of the launch grid lane by lane; the bytes must equal tests/resample_ref.py's resize of tests/rgb_ref.py's to_rgb, the
tensors' bit patterns tests/tensor_ref.py's of that, exactly.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import resample_ref as R
import rgb_ref as G
import tensor_ref as T

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
# the flags of tests/emu/Makefile
_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-DJPGPU_HOST_EMULATION"]
LDS = 32 * 1024  # RS_MAX_LDS
DTYPE_ID = {"float32": 1, "float16": 2, "bfloat16": 3}
GUARD8 = 0xA7
GUARD = {4: 0x5A5A5A5A, 2: 0x5A5A}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("emu_rgb")
    so = str(d / "libemurgb.so")
    cmd = [os.environ.get("CXX", "g++"), *_FLAGS, "-shared", "-I", _EMU, "-include", os.path.join(_EMU, "hip_shim.hpp"), "-o", so,
           os.path.join(_EMU, "emu_rgb.cpp")]
    subprocess.check_call(cmd)
    L = C.CDLL(so)
    L.emu_rgb_resample.argtypes = [C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.emu_rgb_resample.restype = C.c_int
    L.emu_rgb_tensor.argtypes = [C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.emu_rgb_tensor.restype = C.c_int
    L.emu_rgb_plan_ok.argtypes = [C.c_uint32, C.c_uint32]
    L.emu_rgb_plan_ok.restype = C.c_int
    return L


def _source(img, src_off):
    """The image's bytes `src_off` bytes behind a 4-byte aligned address, 0xEE around them -> (keep-alive array, address)."""
    buf = np.full(img.size + src_off + 16, 0xEE, np.uint8)
    skip = -buf.ctypes.data % 4 + src_off
    buf[skip: skip + img.size] = img.reshape(-1)
    return buf, buf.ctypes.data + skip


_INFO = "rb bands cap_rows chunks lds_bytes pitch".split()


def run_u8(lib, img, ow, oh, src_off=0, lds_cap=LDS, rb_cap=64):
    """-> ((oh, ow, 3) u8, info).  The guard bytes behind the output must stay untouched."""
    H, W, snc = img.shape
    assert snc != 4 or src_off == 0  # (a CMYK window row is 4-byte aligned in the product)
    keep, addr = _source(img, src_off)
    raw = np.full(ow * oh * 3 + 64 + 4, GUARD8, np.uint8)
    skip = -raw.ctypes.data % 4
    out = raw[skip: skip + ow * oh * 3 + 64]
    info = np.zeros(8, np.uint32)
    rc = lib.emu_rgb_resample(addr, W, H, snc, ow, oh, out.ctypes.data, lds_cap, rb_cap, info.ctypes.data)
    assert rc == 0, rc
    assert (out[ow * oh * 3:] == GUARD8).all(), "the kernel wrote past the image"
    assert (keep == 0xEE).sum() >= 16, "the source changed"
    return out[: ow * oh * 3].reshape(oh, ow, 3).copy(), dict(zip(_INFO, (int(v) for v in info[:6])))


def run_tensor(lib, img, ow, oh, fmt, flip, src_off=0, lds_cap=LDS, rb_cap=64):
    """-> ((3, oh, ow) bit patterns, info).  The guard elements behind the tensor must stay untouched."""
    H, W, snc = img.shape
    assert snc != 4 or src_off == 0
    dtype, mean, std = fmt
    es = 4 if dtype == "float32" else 2
    keep, addr = _source(img, src_off)
    bt = np.uint32 if es == 4 else np.uint16
    plane = ow * oh
    raw = np.full(3 * plane + 64 + 16, GUARD[es], bt)
    skip = (-raw.ctypes.data % 16) // es
    out = raw[skip: skip + 3 * plane + 64]
    info = np.zeros(8, np.uint32)
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    rc = lib.emu_rgb_tensor(addr, W, H, snc, ow, oh, out.ctypes.data, int(flip), DTYPE_ID[dtype], m.ctypes.data, s.ctypes.data, lds_cap, rb_cap, info.ctypes.data)
    assert rc == 0, rc
    assert (out[3 * plane:] == GUARD[es]).all(), "the kernel wrote past the tensor"
    return out[: 3 * plane].reshape(3, oh, ow).copy(), dict(zip(_INFO, (int(v) for v in info[:6])))


def _img(rng, H, W, nc, kind="noise"):
    if kind == "extremes":
        return np.where(rng.random((H, W, nc)) < 0.5, 0, 255).astype(np.uint8)
    return rng.integers(0, 256, (H, W, nc), dtype=np.uint8)


_WANT = {}


def want_u8(key, img, ow, oh):
    """resize(to_rgb(img)), computed once per image."""
    if key not in _WANT:
        _WANT[key] = R.resize(G.to_rgb(img), ow, oh)
    return _WANT[key]


def offsets_of(snc):
    return (0, 1, 2, 3) if snc != 4 else (0,)


# (H, W, ow, oh): 1 x 1; up; down to an odd size (element items); down to 224 x 224 (four-pixel items)
SHAPES = [(1, 1, 1, 1), (9, 17, 224, 224), (97, 161, 37, 53), (480, 640, 224, 224)]
_IDS = [f"{s[1]}x{s[0]}-{s[2]}x{s[3]}" for s in SHAPES]


@pytest.mark.parametrize("snc", [1, 4, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_u8_kernel_converts_then_resamples(lib, shape, snc):
    H, W, ow, oh = shape
    rng = np.random.default_rng(H * 7 + W * 131 + ow + snc * 1009)
    for kind in ("noise", "extremes") if snc == 4 else ("noise",):
        img = _img(rng, H, W, snc, kind)
        want = want_u8(("u8", shape, snc, kind), img, ow, oh)
        for src_off in offsets_of(snc):
            got, info = run_u8(lib, img, ow, oh, src_off)
            assert info["chunks"] == 1 and info["lds_bytes"] <= LDS and info["pitch"] == (ow * 3 + 3) & ~3, info
            assert np.array_equal(got, want), (shape, snc, kind, src_off, info, np.argwhere(got != want)[:5].tolist())


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
@pytest.mark.parametrize("snc", [1, 4, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=_IDS)
def test_tensor_kernel_converts_then_resamples(lib, shape, snc, dtype):
    H, W, ow, oh = shape
    rng = np.random.default_rng(H * 7 + W * 131 + ow + snc * 1009)
    fmt = (dtype, *T.IMAGENET)
    tab = T.table(fmt, 3)
    for kind in ("noise", "extremes") if snc == 4 else ("noise",):
        img = _img(rng, H, W, snc, kind)
        u8 = want_u8(("u8", shape, snc, kind), img, ow, oh)
        for flip in (False, True):
            want = T.bits(T.to_tensor(u8, tab, flip))
            for src_off in offsets_of(snc):
                got, info = run_tensor(lib, img, ow, oh, fmt, flip, src_off)
                assert info["chunks"] == 1, info
                assert np.array_equal(got, want), (shape, snc, dtype, kind, flip, src_off, info, np.argwhere(got != want)[:5].tolist())
    if snc == 1:  # (a gray image's three planes differ through T[c] only)
        assert not np.array_equal(tab[0], tab[1])


# (H, W, snc): the chunked vertical path — an output row's support does not fit the LDS budget
CHUNKED = [(2000, 24, 1), (1200, 16, 4)]


@pytest.mark.parametrize("case", CHUNKED, ids=["gray-24x2000", "cmyk-16x1200"])
def test_chunked_vertical_path(lib, case):
    H, W, snc = case
    rng = np.random.default_rng(40 + snc)
    img = _img(rng, H, W, snc)
    fmt32, fmt16 = ("float32", *T.HALF), ("bfloat16", *T.CLIP)
    for (ow, oh) in [(2048, 1), (333, 1)]:
        want = want_u8(("chunk", case, ow), img, ow, oh)
        pitch = (ow * 3 + 3) & ~3
        for cap in (LDS, pitch * 2 + 3):  # (the real budget: five rows of 2048 x 3 bytes; and a small one: two rows)
            got, info = run_u8(lib, img, ow, oh, 3 if snc == 1 else 0, lds_cap=cap)
            assert info["cap_rows"] == min(cap // pitch, H) and info["rb"] == 1, info
            if cap != LDS or ow == 2048:
                assert info["chunks"] > 1, info
            assert np.array_equal(got, want), (case, ow, cap, info)
            for fmt in (fmt32, fmt16):
                tab = T.table(fmt, 3)
                for flip in (False, True):
                    gt, info = run_tensor(lib, img, ow, oh, fmt, flip, 1 if snc == 1 else 0, lds_cap=cap)
                    assert np.array_equal(gt, T.bits(T.to_tensor(want, tab, flip))), (case, ow, cap, fmt[0], flip, info)


def test_band_seams_and_short_bands(lib):
    """Bands of 1, 2 and 5 output rows over heights they do not divide: a band's first / last dword shared with its neighbour."""
    rng = np.random.default_rng(5)
    for snc in (1, 4):
        img = _img(rng, 61, 47, snc)
        for (ow, oh) in [(13, 17), (34, 23)]:
            want = R.resize(G.to_rgb(img), ow, oh)
            for rb_cap in (1, 2, 5):
                got, info = run_u8(lib, img, ow, oh, 0, rb_cap=rb_cap)
                assert info["rb"] <= rb_cap, info
                assert np.array_equal(got, want), (snc, ow, oh, rb_cap)
                gt, _ = run_tensor(lib, img, ow, oh, ("float16", *T.IMAGENET), True, 0, rb_cap=rb_cap)
                assert np.array_equal(gt, T.bits(T.to_tensor(want, T.table(("float16", *T.IMAGENET), 3), True)))


def test_planner_takes_source_channels_only_with_three_output_channels(lib):
    """src_nc = 0 is the job as it always was (any nc); 1 and 4 go with nc = 3 only; nothing else is planned."""
    for nc in (1, 2, 3, 4):
        assert lib.emu_rgb_plan_ok(nc, 0) == 1
    for src_nc in (1, 4):
        assert lib.emu_rgb_plan_ok(3, src_nc) == 1
        for nc in (1, 2, 4):
            assert lib.emu_rgb_plan_ok(nc, src_nc) == 0
    for src_nc in (2, 3, 5):
        assert lib.emu_rgb_plan_ok(3, src_nc) == 0
