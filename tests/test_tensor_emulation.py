"""CPU emulation of the tensor kernel (csrc/tensor_band.hpp) against the numpy statement of DESIGN.md §4.11.

tests/emu/emu_tensor.cpp compiles the product's tables, planner and kernel phases with g++ (the flags of tests/emu/Makefile) and runs
every workgroup of the launch grid lane by lane, the kernel's barriers as phase boundaries; the elements' bit patterns must equal
tests/tensor_ref.py's of tests/resample_ref.py's resize exactly.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import resample_ref as R
import tensor_ref as T

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
# the flags of tests/emu/Makefile
_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-DJPGPU_HOST_EMULATION"]
LDS = 32 * 1024  # RS_MAX_LDS
DTYPE_ID = {"float32": 1, "float16": 2, "bfloat16": 3}
GUARD = {4: 0x5A5A5A5A, 2: 0x5A5A}


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("emu_tensor")
    so = str(d / "libemutensor.so")
    cmd = [os.environ.get("CXX", "g++"), *_FLAGS, "-shared", "-I", _EMU, "-include", os.path.join(_EMU, "hip_shim.hpp"), "-o", so,
           os.path.join(_EMU, "emu_tensor.cpp")]
    subprocess.check_call(cmd)
    L = C.CDLL(so)
    L.emu_tensor.argtypes = [C.c_void_p] + [C.c_uint32] * 5 + [C.c_void_p] + [C.c_uint32] * 3 + [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.emu_tensor.restype = C.c_int
    return L


def run(lib, img, ow, oh, fmt, flip, src_off=0, lds_cap=LDS, rb_cap=64, plane_pad=0):
    """-> (tensor (nc, oh, ow) as bit patterns, info dict).  The source starts `src_off` bytes into its buffer; the guard elements
    behind the tensor — and behind every plane with a padded plane pitch — must stay untouched."""
    H, W, nc = img.shape
    dtype, mean, std = fmt
    es = 4 if dtype == "float32" else 2
    src = np.full(img.size + src_off + 8, 0xEE, np.uint8)
    src[src_off: src_off + img.size] = img.reshape(-1)
    plane = ow * oh + plane_pad
    bt = np.uint32 if es == 4 else np.uint16
    raw = np.full(nc * plane + 64 + 16, GUARD[es], bt)
    skip = (-raw.ctypes.data % 16) // es  # (the image's base is 256-byte aligned in the product: 16 is what the stores need)
    out = raw[skip: skip + nc * plane + 64]
    info = np.zeros(8, np.uint32)
    m, s = np.asarray(mean, np.float32), np.asarray(std, np.float32)
    rc = lib.emu_tensor(src.ctypes.data + src_off, W, H, nc, ow, oh, out.ctypes.data, plane if plane_pad else 0, int(flip), DTYPE_ID[dtype],
                        m.ctypes.data, s.ctypes.data, lds_cap, rb_cap, info.ctypes.data)
    assert rc == 0, rc
    assert (out[nc * plane:] == GUARD[es]).all(), "the kernel wrote past the tensor"
    planes = out[: nc * plane].reshape(nc, plane)
    assert (planes[:, ow * oh:] == GUARD[es]).all(), "the kernel wrote between the planes"
    return planes[:, : ow * oh].reshape(nc, oh, ow).copy(), dict(zip("rb bands cap_rows chunks lds_bytes".split(), (int(v) for v in info[:5])))


def want_of(img, ow, oh, fmt, flip):
    return T.bits(T.to_tensor(R.resize(img, ow, oh), T.table(fmt, img.shape[2]), flip))


def _img(rng, H, W, nc, kind="noise"):
    if kind == "extremes":
        return np.where(rng.random((H, W, nc)) < 0.5, 0, 255).astype(np.uint8)
    return rng.integers(0, 256, (H, W, nc), dtype=np.uint8)


def fmt_of(dtype, which=T.IMAGENET):
    return (dtype, which[0], which[1])


# (H, W, ow, oh)
SHAPES = [(108, 192, 22, 22), (17, 23, 224, 224), (53, 80, 23, 21), (1, 1, 8, 8), (64, 64, 1, 1), (5, 5, 2048, 3), (30, 200, 3, 7), (2, 3, 5, 9)]


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("nc", [1, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}-{s[2]}x{s[3]}")
def test_tensor_kernel_logic_matches_the_numpy_statement(lib, shape, nc, dtype):
    H, W, ow, oh = shape
    rng = np.random.default_rng(H * 7 + W * 131 + ow + nc * 1009)
    fmt = fmt_of(dtype)
    for kind in ("noise", "extremes"):
        img = _img(rng, H, W, nc, kind)
        for flip in (False, True):
            want = want_of(img, ow, oh, fmt, flip)
            for src_off in (0, 1, 2, 3):  # (source rows at every byte alignment)
                got, info = run(lib, img, ow, oh, fmt, flip, src_off)
                assert info["chunks"] == 1 and info["lds_bytes"] <= LDS, info
                assert np.array_equal(got, want), (shape, nc, dtype, kind, flip, src_off, info, np.argwhere(got != want)[:5].tolist())


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("nc", [1, 3, 4])
def test_items_shared_at_band_and_plane_seams(lib, nc, dtype):
    """Bands of 1, 2, 3, 5 and 7 output rows over heights they do not divide, out_w % 4 in {0, 1, 2, 3}: where a band's run of a plane
    does not start or end at a multiple of four elements it shares an item with its neighbour — or with the next plane — and each
    stores its own elements.  With a padded plane pitch nothing between the planes is written."""
    rng = np.random.default_rng(nc)
    fmt = fmt_of(dtype, T.CLIP)
    for (H, W, ow, oh) in [(61, 47, 13, 17), (40, 40, 20, 23), (9, 100, 34, 23), (233, 10, 7, 11)]:
        img = _img(rng, H, W, nc)
        for flip in (False, True):
            want = want_of(img, ow, oh, fmt, flip)
            for rb_cap in (1, 2, 3, 5, 7):
                for plane_pad in (0, 4, 5):
                    got, info = run(lib, img, ow, oh, fmt, flip, 1, rb_cap=rb_cap, plane_pad=plane_pad)
                    assert info["rb"] <= rb_cap and info["bands"] == -(-oh // info["rb"]), info
                    assert np.array_equal(got, want), (H, W, ow, oh, flip, rb_cap, plane_pad, info)


@pytest.mark.parametrize("dtype", T.DTYPES)
@pytest.mark.parametrize("nc", [1, 3, 4])
def test_chunked_vertical_path(lib, nc, dtype):
    """An LDS budget of a few rows: an output row's support takes several chunks, the sums gathered in registers group by group."""
    rng = np.random.default_rng(40 + nc)
    fmt = fmt_of(dtype, T.HALF)
    for (H, W, ow, oh) in [(300, 20, 9, 2), (64, 64, 64, 5), (1200, 16, 2048, 1), (97, 400, 300, 3), (60, 30, 1030, 2)]:
        img = _img(rng, H, W, nc)
        pitch = (ow * nc + 3) & ~3
        for flip in (False, True):
            want = want_of(img, ow, oh, fmt, flip)
            for rows in (1, 2, 5):
                got, info = run(lib, img, ow, oh, fmt, flip, 3, lds_cap=pitch * rows + 3)
                assert info["cap_rows"] == min(rows, H, LDS // pitch), info
                if oh < H or rows == 1:
                    assert info["chunks"] > 1 and info["rb"] == 1, info
                assert np.array_equal(got, want), (H, W, ow, oh, nc, flip, rows, info)
    # the real budget: 2048 x 4-byte rows leave four source rows per chunk
    img = _img(rng, 1200, 16, 4)
    for flip in (False, True):
        got, info = run(lib, img, 2048, 1, fmt, flip)
        assert info["cap_rows"] == 4 and info["chunks"] == 300, info
        assert np.array_equal(got, want_of(img, 2048, 1, fmt, flip))


def test_two_channels_and_other_formats(lib):
    """nc = 2 (the fourth instance of the four-pixel item) and formats whose table holds infinities, negative values and zeros."""
    rng = np.random.default_rng(9)
    tiny = ((0.25, -3.0, 0.0, 0.0), (1e-30, 2.0, 1.0, 1.0))
    for nc in (1, 2, 3, 4):
        for (H, W, ow, oh) in [(20, 30, 16, 9), (20, 30, 15, 9)]:
            img = _img(rng, H, W, nc)
            for dtype in T.DTYPES:
                for which in (T.IDENTITY, tiny):
                    fmt = fmt_of(dtype, which)
                    for flip in (False, True):
                        got, _info = run(lib, img, ow, oh, fmt, flip, 2)
                        assert np.array_equal(got, want_of(img, ow, oh, fmt, flip)), (nc, ow, dtype, flip)
