"""The fixed-output stage of a batch as csrc/batch_output.hpp states it, without a GPU: the options record, the rule function, the
placement normalisation, the bytes per image and the route, compiled with g++ (tests/emu/emu_batch_output.cpp) and checked against the
rules as include/jpgpu.h and DESIGN.md §4.10-4.16 state them — the statuses below are those jpgpu_batch_create* returns, which the
refusal tests of the GPU suite assert through the library."""
import ctypes as C
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import jpeg_decoder_amd as J

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_EMU = os.path.join(ROOT, "tests", "emu")
# the flags of tests/emu/Makefile
_FLAGS = ["-std=c++17", "-Wall", "-Wno-unknown-pragmas", "-Wno-unused-function", "-DJPGPU_HOST_EMULATION"]
OK, ERR_FORMAT, ERR_UNSUPPORTED = 0, 1, 2
N = J._native
MAX_OUT = 2048


class Spec(C.Structure):
    """struct EmuSpec (tests/emu/emu_batch_output.cpp): OutputSpec with plain fields."""
    _fields_ = [("w", C.c_uint32), ("h", C.c_uint32), ("filter", C.c_uint32), ("rgb", C.c_uint32), ("tensor", C.c_uint32),
                ("tn", N.TensorFormatStruct), ("fill", C.c_uint8 * 4), ("warp", C.c_uint32), ("wp", N.WarpOptionsStruct)]


def spec(size=(0, 0), filter=0, rgb=False, dtype=None, tn_reserved=0, mean=(0, 0, 0, 0), std=(1, 1, 1, 1), fill=(0, 0, 0, 0), warp=None, wfill=(0, 0, 0, 0),
         wp_reserved=0):
    """dtype None: no tensor format; warp None: no warp options (an absent option holds zeros, as the Pipeline's setters store it)."""
    s = Spec()
    s.w, s.h, s.filter, s.rgb = size[0], size[1], filter, int(rgb)
    s.fill[:] = fill
    if dtype is not None:
        s.tensor, s.tn.dtype, s.tn.reserved = 1, dtype, tn_reserved
        s.tn.mean[:], s.tn.std[:] = mean, std
    if warp is not None:
        s.warp, s.wp.filter, s.wp.reserved = 1, warp, wp_reserved
        s.wp.fill[:] = wfill
    return s


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("emu_batch_output") / "libemuoutput.so")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-O2", "-fPIC", *_FLAGS, "-shared", "-I", _EMU, "-include", os.path.join(_EMU, "hip_shim.hpp"), "-o", so,
                           os.path.join(_EMU, "emu_batch_output.cpp"), os.path.join(ROOT, "jpeg-decoder_amd", "csrc", "image_job.cpp")])
    L = C.CDLL(so)
    L.emu_output_rule.argtypes = [C.c_void_p, C.c_char_p, C.c_uint32]
    L.emu_output_image_rule.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_char_p, C.c_uint32]
    L.emu_spec_equal.argtypes = [C.c_void_p, C.c_void_p]
    L.emu_spec_is_default.argtypes = [C.c_void_p]
    L.emu_normalise_placements.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_void_p, C.c_void_p]
    L.emu_normalise_placements.restype = C.c_uint32
    L.emu_placed_axis.argtypes = [C.c_uint32, C.c_int32, C.c_uint32, C.c_void_p]
    L.emu_output_image_bytes.argtypes = [C.c_void_p, C.c_uint32, C.c_int]
    L.emu_output_image_bytes.restype = C.c_size_t
    L.emu_output_arena.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p, C.c_void_p]
    L.emu_output_arena.restype = C.c_size_t
    L.emu_output_route.argtypes = [C.c_void_p, C.c_int, C.c_uint32, C.c_void_p]
    L.emu_cc_none.restype = C.c_uint32
    L.emu_rs_max_out.restype = C.c_uint32
    assert L.emu_rs_max_out() == MAX_OUT
    return L


def _rule(lib, s):
    why = C.create_string_buffer(300)
    rc = lib.emu_output_rule(C.byref(s), why, 300)
    return rc, why.value.decode()


SIZES = {"none": (0, 0), "valid": (8, 8), "0xh": (0, 8), "2049": (2049, 8)}
FILTERS = (0, 3, 9)
TENSORS = {"none": None, "f16": N.TENSOR_F16, "dtype 0": 0}
WARPS = {"none": None, "bilinear": N.WARP_BILINEAR, "filter 2": 2}


def _expected(size, filter, rgb, tensor, warp):
    """The status and a word of the reason, in the order jpgpu_batch_create* checks: the size's range, the filter's id, then what needs an
    output size (a filter or the RGB flag without one: UNSUPPORTED — the flags mean nothing there; the rest: FORMAT), the warp options, the
    tensor format's dtype."""
    sized = SIZES[size] != (0, 0)
    if size in ("0xh", "2049"):
        return ERR_FORMAT, "output size"
    if filter > 4:
        return ERR_FORMAT, f"filter {filter}"
    if filter and not sized:
        return ERR_UNSUPPORTED, "output size"
    if rgb and not sized:
        return ERR_UNSUPPORTED, "output size"
    if warp != "none" and not sized:
        return ERR_FORMAT, "output size"
    if warp == "filter 2":
        return ERR_FORMAT, "warp options"
    if tensor != "none" and not sized:
        return ERR_FORMAT, "output size"
    if tensor == "dtype 0":
        return ERR_FORMAT, "tensor"
    return OK, ""


def _check_the_rule_function_over_the_cross_of_options(lib):
    seen = {OK: 0, ERR_FORMAT: 0, ERR_UNSUPPORTED: 0}
    for size, filter, rgb, tensor, warp in itertools.product(SIZES, FILTERS, (False, True), TENSORS, WARPS):
        rc, why = _rule(lib, spec(SIZES[size], filter, rgb, TENSORS[tensor], warp=WARPS[warp]))
        want, word = _expected(size, filter, rgb, tensor, warp)
        assert rc == want and word in why and (rc != OK or why == ""), (size, filter, rgb, tensor, warp, rc, why)
        seen[rc] += 1
    assert sum(seen.values()) == 4 * 3 * 2 * 3 * 3 and seen[OK] == 1 * 2 * 2 * 2 * 2 + 1 and min(seen.values()) > 0  # (valid size; no size with no option)
    # the reasons keep the words callers match
    assert "bicubic" in _rule(lib, spec(filter=3))[1] and "1..2048" in _rule(lib, spec((8, 2049)))[1]
    assert _rule(lib, spec((MAX_OUT, MAX_OUT))) == (OK, "") and _rule(lib, spec((1, 1), filter=4, warp=0)) == (OK, "")
    assert _rule(lib, spec((8, 8), dtype=N.TENSOR_F32, tn_reserved=1))[0] == ERR_FORMAT and _rule(lib, spec((8, 8), dtype=4))[0] == ERR_FORMAT
    assert _rule(lib, spec((8, 8), warp=0, wp_reserved=1))[0] == ERR_FORMAT


def _check_the_rule_per_image(lib):
    cc_none, cc_other = lib.emu_cc_none(), lib.emu_cc_none() + 1

    def rule(s, ncomp, fn=cc_other):
        why = C.create_string_buffer(300)
        return lib.emu_output_image_rule(C.byref(s), ncomp, fn, why, 300), why.value.decode()

    for nc in (1, 2, 3, 4):  # without an output size nothing is refused, planar output included
        assert rule(spec(), nc, cc_none) == (OK, "")
    assert rule(spec((8, 8)), 1, cc_none) == (OK, "")  # (one component is not planar)
    for nc in (2, 3, 4):
        rc, why = rule(spec((8, 8)), nc, cc_none)
        assert rc == ERR_UNSUPPORTED and "planar" in why
        assert rule(spec((8, 8)), nc) == (OK, "")
    for nc, want in ((1, OK), (2, ERR_UNSUPPORTED), (3, OK), (4, OK)):  # RGB output: gray, three components, CMYK
        rc, why = rule(spec((8, 8), rgb=True), nc)
        assert rc == want and (rc == OK or "RGB" in why)
    # the tensor format against the image's channels: a channel the image has not is not looked at; with RGB output there are three
    for bad in (0.0, float("nan"), float("inf")):
        fmt = dict(dtype=N.TENSOR_F16, std=(0.5, 0.5, bad, 1))
        assert rule(spec((8, 8), **fmt), 1) == (OK, "") and rule(spec((8, 8), **fmt), 4)[0] == ERR_FORMAT
        rc, why = rule(spec((8, 8), **fmt), 3)
        assert rc == ERR_FORMAT and "tensor" in why and "std" in why
        assert rule(spec((8, 8), rgb=True, **fmt), 1)[0] == ERR_FORMAT
    rc, why = rule(spec((8, 8), dtype=N.TENSOR_F32, mean=(float("nan"), 0, 0, 0)), 1)
    assert rc == ERR_FORMAT and "mean" in why


def _check_spec_equality_is_field_by_field(lib):
    base = dict(size=(8, 6), filter=2, rgb=True, dtype=N.TENSOR_F16, mean=(0.1, 0.2, 0.3, 0.4), std=(1, 2, 3, 4), fill=(1, 2, 3, 4), warp=1, wfill=(5, 6, 7, 8))
    changes = [dict(size=(9, 6)), dict(size=(8, 7)), dict(filter=3), dict(rgb=False), dict(dtype=None), dict(dtype=N.TENSOR_BF16), dict(tn_reserved=1),
               dict(warp=None), dict(warp=0), dict(wp_reserved=1)]
    changes += [dict(mean=tuple(0.5 if k == c else v for k, v in enumerate(base["mean"]))) for c in range(4)]
    changes += [dict(std=tuple(0.5 if k == c else v for k, v in enumerate(base["std"]))) for c in range(4)]
    changes += [dict(fill=tuple(9 if k == c else v for k, v in enumerate(base["fill"]))) for c in range(4)]
    changes += [dict(wfill=tuple(9 if k == c else v for k, v in enumerate(base["wfill"]))) for c in range(4)]
    a = spec(**base)
    assert lib.emu_spec_equal(C.byref(a), C.byref(spec(**base))) == 1
    for ch in changes:
        b = spec(**{**base, **ch})
        assert lib.emu_spec_equal(C.byref(a), C.byref(b)) == 0 and lib.emu_spec_equal(C.byref(b), C.byref(a)) == 0, ch
        assert lib.emu_spec_equal(C.byref(b), C.byref(spec(**{**base, **ch}))) == 1, ch
    # padding plays no part: the same fields in memory of another colour compare equal
    noisy = Spec()
    C.memset(C.byref(noisy), 0xA5, C.sizeof(noisy))
    for name, _ in Spec._fields_:
        setattr(noisy, name, getattr(a, name))
    assert lib.emu_spec_equal(C.byref(a), C.byref(noisy)) == 1
    # an absent option is its zero value
    assert lib.emu_spec_is_default(C.byref(spec())) == 1 and lib.emu_spec_is_default(C.byref(spec((1, 1)))) == 0


def _visible(r, at, out):
    lo, hi = max(at, 0), min(at + r, out)
    return r != 0 and lo < hi


def _normalise(lib, pls, w, h):
    arr = (N.Placement * len(pls))(*[N.Placement(*p) for p in pls])
    out = (N.Placement * len(pls))()
    placed = C.c_uint32(7)
    k = lib.emu_normalise_placements(arr, len(pls), w, h, out, C.byref(placed))
    return k, bool(placed.value), [(o.rw, o.rh, o.x, o.y) for o in out]


def _check_placement_normalisation(lib):
    W, H = 12, 8
    # none — in both spellings — and the identity: written out as the whole output, the batch stays unplaced
    k, placed, out = _normalise(lib, [(0, 0, 0, 0), (0, 5, 3, 3), (5, 0, -3, 9), (W, H, 0, 0)], W, H)
    assert (k, placed) == (4, False) and out == [(W, H, 0, 0)] * 4
    # partly outside: kept as given, and the batch is a placed one; so is a placement of another size or at another place
    for pl in [(20, 20, -5, -7), (W, H, 1, 0), (W, H, 0, -1), (W - 1, H, 0, 0), (W, H + 1, 0, 0), (1, 1, W - 1, H - 1), (65535, 65535, -65534, -65534)]:
        k, placed, out = _normalise(lib, [(0, 0, 0, 0), pl], W, H)
        assert (k, placed) == (2, True) and out == [(W, H, 0, 0), pl], pl
    # wholly outside: the index of the first such image
    for pl in [(4, 4, W, 0), (4, 4, -4, 0), (4, 4, 0, H), (4, 4, 0, -4), (65535, 1, -65535, 0), (1, 1, 2 ** 31 - 1, 0), (1, 1, -2 ** 31, 0)]:
        assert _normalise(lib, [(0, 0, 0, 0), (3, 3, 1, 1), pl, pl], W, H)[0] == 2, pl
        assert _normalise(lib, [pl], W, H)[0] == 0
    # visibility is placed_axis's (csrc/placed_band.hpp), which is the statement of include/jpgpu.h: x < out_w, x + rw > 0
    rng = np.random.default_rng(5)
    out3 = (C.c_uint32 * 3)()
    seen = [0, 0]
    for _ in range(3000):
        rw, rh = (int(v) for v in rng.integers(1, 40, 2))
        x, y = (int(v) for v in rng.integers(-45, 20, 2))
        want = _visible(rw, x, W) and _visible(rh, y, H)
        assert (_normalise(lib, [(rw, rh, x, y)], W, H)[0] == 1) == want
        assert bool(lib.emu_placed_axis(rw, x, W, out3)) == _visible(rw, x, W) and bool(lib.emu_placed_axis(rh, y, H, out3)) == _visible(rh, y, H)
        seen[want] += 1
    assert min(seen) > 300


def _check_output_bytes_per_image(lib):
    for (w, h), rgb, nc in itertools.product([(8, 8), (224, 224), (1, 2048), (2048, 2048), (13, 7)], (False, True), (1, 3, 4)):
        ch = 3 if rgb else nc
        for dtype, es in ((None, 1), (N.TENSOR_F32, 4), (N.TENSOR_F16, 2), (N.TENSOR_BF16, 2)):
            s = spec((w, h), rgb=rgb, dtype=dtype, warp=None if dtype == N.TENSOR_F16 else 1)
            assert lib.emu_output_image_bytes(C.byref(s), nc, 0) == w * h * ch * es
            assert lib.emu_output_image_bytes(C.byref(s), nc, 1) == w * h * ch  # (the warp's source: what the u8 batch's output would be)
    # laid out as every arena is: 256-byte aligned running offsets, at least 256 bytes
    ncomps = np.array([3, 1, 4, 3, 1], np.uint32)
    for s, u8 in ((spec((13, 7), dtype=N.TENSOR_F16), 0), (spec((13, 7), dtype=N.TENSOR_F16, warp=0), 1), (spec((224, 224), rgb=True, dtype=N.TENSOR_F32), 0),
                  (spec((1, 1)), 0)):
        off, ln = np.zeros(5, np.uint64), np.zeros(5, np.uint64)
        total = lib.emu_output_arena(C.byref(s), ncomps.ctypes.data, 5, u8, off.ctypes.data, ln.ctypes.data)
        want = [lib.emu_output_image_bytes(C.byref(s), int(nc), u8) for nc in ncomps]
        assert list(ln) == want
        at = 0
        for i, b in enumerate(want):
            assert off[i] == at
            at += (b + 255) // 256 * 256
        assert total == max(at, 256)
    s = spec((224, 224), rgb=True, dtype=N.TENSOR_F32)  # (N images of 3 x 224 x 224 follow each other without a gap)
    off, ln = np.zeros(5, np.uint64), np.zeros(5, np.uint64)
    assert lib.emu_output_arena(C.byref(s), ncomps.ctypes.data, 5, 0, off.ctypes.data, ln.ctypes.data) == 5 * 3 * 224 * 224 * 4


NONE, BAND, TENSOR, PLACED, PLACED_TENSOR = range(5)


def _check_the_route_table(lib):
    out4 = (C.c_uint32 * 4)()
    for placed, tensor, warp, runs in itertools.product((False, True), (False, True), (False, True), (0, 3)):
        s = spec((8, 8), dtype=N.TENSOR_F16 if tensor else None, warp=1 if warp else None)
        lib.emu_output_route(C.byref(s), int(placed), runs, out4)
        resample, has_runs, has_warp, tensor_jobs = out4
        # a warped batch resamples to u8, whatever it writes in the end
        rs_tensor = tensor and not warp
        want = {(False, False): BAND, (False, True): TENSOR, (True, False): PLACED, (True, True): PLACED_TENSOR}[(placed, rs_tensor)]
        assert resample == want and bool(has_warp) == warp and bool(tensor_jobs) == rs_tensor, (placed, tensor, warp, runs)
        assert bool(has_runs) == (runs != 0 and not placed)  # (runs of bands: never with placements)
    for placed, runs in itertools.product((False, True), (0, 3)):  # no output size: no launch at all
        lib.emu_output_route(C.byref(spec()), int(placed), runs, out4)
        assert list(out4) == [NONE, 0, 0, 0]


def test_the_header_against_the_rules_as_stated(lib):
    """One test for the header's six parts, each a function above: the parts share the compiled library and none takes a tenth of a second."""
    _check_the_rule_function_over_the_cross_of_options(lib)
    _check_the_rule_per_image(lib)
    _check_spec_equality_is_field_by_field(lib)
    _check_placement_normalisation(lib)
    _check_output_bytes_per_image(lib)
    _check_the_route_table(lib)


def test_the_header_under_the_sanitizers(tmp_path):
    """A stand-alone program (its own main): nothing is loaded into Python."""
    cxx = shutil.which(os.environ.get("CXX", "g++"))
    if cxx is None:
        pytest.skip("no C++ compiler")
    exe = str(tmp_path / "batch_output_asan")
    subprocess.check_call([cxx, "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-g", "-O1", *_FLAGS, "-I", _EMU, "-include",
                           os.path.join(_EMU, "hip_shim.hpp"), "-o", exe, os.path.join(_EMU, "batch_output_asan.cpp"),
                           os.path.join(ROOT, "jpeg-decoder_amd", "csrc", "image_job.cpp")])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "batch_output_asan: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
