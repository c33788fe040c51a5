"""CPU emulation of the resample kernel (csrc/resample_band.hpp) against the numpy statement of DESIGN.md §4.10.

tests/emu/emu_resample.cpp compiles the product's tables, planner and kernel phases with g++ (the flags of tests/emu/Makefile) and runs
every workgroup of the launch grid lane by lane, the kernel's barriers as phase boundaries; the bytes must equal
tests/resample_ref.py's exactly.  No GPU needed."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import resample_ref as R

_HERE = os.path.dirname(os.path.abspath(__file__))
_EMU = os.path.join(_HERE, "emu")
_CSRC = os.path.join(os.path.dirname(_HERE), "jpeg-decoder_amd", "csrc")
# the flags of tests/emu/Makefile
_FLAGS = ["-O2", "-std=c++17", "-fPIC", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-DJPGPU_HOST_EMULATION"]
LDS = 32 * 1024  # RS_MAX_LDS


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("emu_resample")
    so = str(d / "libemuresample.so")
    cmd = [os.environ.get("CXX", "g++"), *_FLAGS, "-shared", "-I", _EMU, "-include", os.path.join(_EMU, "hip_shim.hpp"), "-o", so,
           os.path.join(_EMU, "emu_resample.cpp")]
    subprocess.check_call(cmd)
    L = C.CDLL(so)
    L.emu_resample.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p]
    L.emu_resample.restype = C.c_int
    L.emu_resample_ksize.argtypes = [C.c_uint32, C.c_uint32]
    L.emu_resample_ksize.restype = C.c_uint32
    L.emu_resample_coefficients.argtypes = [C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p, C.c_uint32]
    return L


def run(lib, img, ow, oh, src_off=0, lds_cap=LDS, rb_cap=64):
    """-> (out (oh, ow, nc), info dict).  The source starts `src_off` bytes into its buffer (window rows start anywhere); a guard band
    behind the output must stay untouched."""
    H, W, nc = img.shape
    src = np.full(img.size + src_off + 8, 0xEE, np.uint8)
    src[src_off: src_off + img.size] = img.reshape(-1)
    n = ow * oh * nc
    out = np.full(n + 64, 0x5A, np.uint8)
    info = np.zeros(8, np.uint32)
    rc = lib.emu_resample(src.ctypes.data + src_off, W, H, nc, ow, oh, out.ctypes.data, lds_cap, rb_cap, info.ctypes.data)
    assert rc == 0, rc
    assert (out[n:] == 0x5A).all(), "the kernel wrote past the image's bytes"
    return out[:n].reshape(oh, ow, nc), dict(zip("rb bands cap_rows chunks lds_bytes".split(), (int(v) for v in info[:5])))


def _img(rng, H, W, nc, kind="noise"):
    if kind == "extremes":  # (0 / 255 only: the rounding and the clamp at both ends)
        return np.where(rng.random((H, W, nc)) < 0.5, 0, 255).astype(np.uint8)
    return rng.integers(0, 256, (H, W, nc), dtype=np.uint8)


def test_tables_are_the_numpy_tables(lib):
    for in_size, out_size in [(1, 1), (1, 2048), (65535, 1), (1080, 224), (224, 224), (997, 13), (13, 997), (540, 224), (3, 7), (2039, 251)]:
        ks = lib.emu_resample_ksize(in_size, out_size)
        wb, wk = R.coefficients(in_size, out_size)
        assert ks == wk.shape[1]
        b, k = np.full((out_size, 2), -1, np.int32), np.full((out_size, ks), -1, np.int32)
        lib.emu_resample_coefficients(in_size, out_size, b.ctypes.data, k.ctypes.data, ks)
        assert np.array_equal(b, wb) and np.array_equal(k, wk), (in_size, out_size)


# (H, W, ow, oh): down-scaling, up-scaling, mixed, the identity, one pixel in / out, rows of 2048 pixels, odd row lengths
SHAPES = [(108, 192, 22, 22), (540, 960, 224, 224), (17, 23, 224, 224), (50, 50, 50, 50), (53, 80, 23, 21), (97, 131, 25, 19), (1, 1, 8, 8),
          (200, 30, 7, 3), (64, 64, 1, 1), (5, 5, 2048, 3), (30, 200, 3, 7), (31, 33, 33, 31), (2, 3, 5, 9), (300, 7, 9, 2)]


@pytest.mark.parametrize("nc", [1, 3, 4])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[1]}x{s[0]}-{s[2]}x{s[3]}")
def test_resample_kernel_logic_matches_the_numpy_statement(lib, shape, nc):
    H, W, ow, oh = shape
    rng = np.random.default_rng(H * 7 + W * 131 + ow + nc * 1009)
    for kind in ("noise", "extremes"):
        img = _img(rng, H, W, nc, kind)
        want = R.resize(img, ow, oh)
        for src_off in (0, 1, 2, 3):  # (source rows at every byte alignment)
            got, info = run(lib, img, ow, oh, src_off)
            assert info["chunks"] == 1 and info["lds_bytes"] <= LDS, info
            assert np.array_equal(got, want), (shape, nc, kind, src_off, info, np.argwhere(got != want)[:5].tolist())


@pytest.mark.parametrize("nc", [1, 3, 4])
def test_bands_at_the_image_edges_and_of_every_height(lib, nc):
    """Bands of 1, 2, 3, 5 and 7 output rows over heights they do not divide: the first band starts at source row 0, the last one ends
    with the image, and where out_w * nc is no multiple of four neighbouring bands share a destination dword (each stores its own
    bytes of it)."""
    rng = np.random.default_rng(nc)
    for (H, W, ow, oh) in [(61, 47, 13, 17), (40, 40, 21, 40), (9, 100, 33, 23), (233, 10, 7, 11)]:
        img = _img(rng, H, W, nc)
        want = R.resize(img, ow, oh)
        for rb_cap in (1, 2, 3, 5, 7):
            got, info = run(lib, img, ow, oh, 1, rb_cap=rb_cap)
            assert info["rb"] <= rb_cap and info["bands"] == -(-oh // info["rb"]), info
            assert np.array_equal(got, want), (H, W, ow, oh, rb_cap, info)


@pytest.mark.parametrize("nc", [1, 3, 4])
def test_chunked_vertical_path(lib, nc):
    """An LDS budget of a few rows: an output row's support takes several chunks, the sums gathered in registers group by group (rows
    wider than RS_NT dwords have several groups)."""
    rng = np.random.default_rng(40 + nc)
    for (H, W, ow, oh) in [(300, 20, 9, 2), (64, 64, 64, 5), (1200, 16, 2048, 1), (97, 400, 300, 3), (50, 50, 50, 50)]:
        for kind in ("noise", "extremes"):
            img = _img(rng, H, W, nc, kind)
            want = R.resize(img, ow, oh)
            pitch = (ow * nc + 3) & ~3
            for rows in (1, 2, 5):
                got, info = run(lib, img, ow, oh, 3, lds_cap=pitch * rows + 3)
                assert info["cap_rows"] == min(rows, H, LDS // pitch), info  # (never more than the real budget)
                if oh < H or rows == 1:
                    assert info["chunks"] > 1 and info["rb"] == 1, info
                assert np.array_equal(got, want), (H, W, ow, oh, nc, kind, rows, info)
    # the real budget: 2048 x 4-byte rows leave four source rows per chunk
    img = _img(rng, 1200, 16, 4)
    got, info = run(lib, img, 2048, 1)
    assert info["cap_rows"] == 4 and info["chunks"] == 300, info
    assert np.array_equal(got, R.resize(img, 2048, 1))


def test_the_identity(lib):
    rng = np.random.default_rng(5)
    for nc in (1, 3, 4):
        for (H, W) in [(1, 1), (37, 53), (224, 224), (3, 2048)]:
            img = _img(rng, H, W, nc)
            got, _info = run(lib, img, W, H, 2)
            assert np.array_equal(got, img)


def test_planner_fits_its_budget(lib):
    """Every plan's LDS footprint stays within RS_MAX_LDS and a band's source rows within one chunk wherever a single row's do."""
    rng = np.random.default_rng(6)
    for _ in range(40):
        H, W, nc = int(rng.integers(1, 400)), int(rng.integers(1, 300)), int(rng.choice([1, 3, 4]))
        ow, oh = int(rng.integers(1, 2049)), int(rng.integers(1, 40))
        img = _img(rng, H, W, nc)
        got, info = run(lib, img, ow, oh)
        assert info["lds_bytes"] <= LDS and info["lds_bytes"] == info["cap_rows"] * ((ow * nc + 3) & ~3), info
        assert info["chunks"] == 1 or info["rb"] == 1, info
        assert np.array_equal(got, R.resize(img, ow, oh)), (H, W, nc, ow, oh, info)
