"""Colour operations (jpgpu_batch_create_coloured, csrc/colour_band.hpp) on the MI355X: every image's u8 result of the fixed output
size through a program of Pillow operations of its own, before the warp and the tensor table.  The expected value is always
tests/colour_ref.py (the numpy statement of DESIGN.md §4.20, pinned to Pillow by tests/golden/colour) applied to the reference result
the resize, filter, placement, RGB, warp and tensor tests use, compared with np.array_equal."""
import ctypes as C

import numpy as np
import pytest

import colour_ref as CR
import filter_ref as F
import rgb_ref as G
import tensor_ref as T
import test_gpu_pipeline_windows as PW
import test_gpu_resize as RZ
import test_gpu_tensor as TN
import warp_ref as WR
from stream_harness import StreamHarness

pytestmark = pytest.mark.gpu

J = None
PFILL, WFILL = (114, 7, 200, 33), (9, 250, 77, 140)
L420, L444, LGRAY, LCMYK = ([(2, 2), (1, 1), (1, 1)], "YCbCr"), ([(1, 1)] * 3, "YCbCr"), ([(1, 1)], "Grayscale"), ([(1, 1)] * 4, "CMYK")
SIZES = [(16, 16), (33, 17), (224, 224), (2048, 64)]
REFTEST_RGB = ["mozilla/jpg-size-33x33.jpg", "mozilla/jpg-size-17x17.jpg", "restarts.jpg", "non-interleaved-mcu.jpg", "mozilla/jpg-progressive.jpg"]
REFTEST_OTHER = ["mozilla/jpg-gray.jpg", "mozilla/jpg-cmyk-1.jpg"]

ALONE = [[("brightness", 0.37)], [("brightness", 1.9)], [("contrast", 0.37)], [("contrast", 1.9)], [("contrast", 0.0)], [("saturation", 0.0)], [("saturation", 0.37)],
         [("saturation", 1.9)], [("saturation", 1.0)], [("solarize", 128)], [("solarize", 0)], [("solarize", 256)], [("posterize", 1)], [("posterize", 4)],
         [("posterize", 8)], [("invert", 0)], [("autocontrast", 0)], [("equalize", 0)], [("identity", 0)], [("brightness", 0.0)], [("brightness", 1.0)]]
MIXED = [[("brightness", 1.9), ("autocontrast", 0)], [("saturation", 0.37), ("equalize", 0)],
         [("solarize", 128), ("contrast", 1.9), ("saturation", 0.0), ("autocontrast", 0)], [("posterize", 3), ("saturation", 1.9), ("contrast", 0.37)],
         [("invert", 0), ("equalize", 0), ("brightness", 0.37)], [("contrast", 0.37), ("autocontrast", 0), ("equalize", 0), ("saturation", 1.9)]]
PROGRAMS = ALONE + MIXED + [None, []]


@pytest.fixture(scope="module", autouse=True)
def _load():
    global J
    import jpeg_decoder_amd as pkg
    J = pkg
    PW.J = pkg
    RZ.J = pkg
    TN.J = pkg
    assert J.device_count() >= 1, "no MI355X visible: the HIP path has no CPU fallback"


_SOURCES = {}


def _synthetic(rng, w, h, layout):
    case = RZ._case(rng, w, h, *layout)
    return {"desc": RZ._desc(case), "coefs": case[2], "src": RZ.source_of(case, RZ._full(case), None)}


def _reftest(rel):
    data = PW._golden("reftest", *rel.split("/"))
    desc, coefs = J.Decoder(data, device=-1).decode_coefficients()
    full, W, H, nc = PW._want(data, None, None)
    return {"desc": desc, "coefs": coefs, "src": full.reshape(H, W, nc)}


def sources(kind):
    """'rgb': three-component sources — the small reftest files, synthetic 4:2:0 and 4:4:4 images of 48 x 40 and 131 x 67; 'other': gray
    and CMYK ones, reftest and synthetic.  Each with the oracle's decode, made once."""
    if not _SOURCES:
        rng = np.random.default_rng(420)
        _SOURCES["rgb"] = [_reftest(r) for r in REFTEST_RGB] + [_synthetic(rng, w, h, lay) for (w, h) in ((48, 40), (131, 67)) for lay in (L420, L444)]
        _SOURCES["other"] = [_reftest(r) for r in REFTEST_OTHER] + [_synthetic(rng, w, h, lay) for (w, h), lay in (((48, 40), LGRAY), ((131, 67), LCMYK), ((131, 67), LGRAY))]
    return _SOURCES[kind]


def pick(kind, n):
    s = sources(kind)
    return [s[i % len(s)] for i in range(n)]


def letterbox(size, i):
    """A placement that pads (the fill shows, is counted by the statistics and is recoloured) for every other image."""
    w, h = size
    return None if i % 2 else (max(1, (2 * w) // 3), max(1, h - 2), w // 6, 1)


_R = {}


def resized_u8(s, size, name=None, rgb=False, pl=None):
    """R: the image's u8 result without colour (cached: the tests share the references)."""
    key = (id(s), size, name, rgb, pl)
    if key not in _R:
        src = G.to_rgb(s["src"]) if rgb else s["src"]
        f = F.NAMES[name or "bilinear"]
        _R[key] = F.resize(src, size[0], size[1], f) if pl is None else F.placed(src, *pl, size[0], size[1], PFILL, f)
    return _R[key]


def want_u8(r, program, flip=False, warp=None, m=None):
    c = CR.apply(r, program) if r.shape[2] == 3 else r
    c = c[:, ::-1] if flip else c
    if warp is None:
        return np.ascontiguousarray(c)
    return WR.warp(c, WR.IDENTITY if m is None else m, WR.BILINEAR if warp == "bilinear" else WR.NEAREST, WFILL)


def upload(b, srcs):
    for i, s in enumerate(srcs):
        for c, a in enumerate(s["coefs"]):
            b.upload(i, c, a)


def batch_of(srcs, size, name=None, fmt=None, rgb=False, pls=None, warp=None, flags=0, colour=True):
    return J.Batch([s["desc"] for s in srcs], flags=flags, output_size=size, tensor=fmt, rgb=rgb, placements=pls, fill=PFILL, filter=name,
                   warp=None if warp is None else J.WarpOptions(warp, WFILL), colour=colour)


def run(srcs, size, programs, name=None, fmt=None, flips=None, rgb=False, pls=None, warp=None, warps=None):
    b = batch_of(srcs, size, name, fmt, rgb, pls, warp)
    try:
        upload(b, srcs)
        b.set_colour(programs)
        if warps is not None:
            b.set_warps(warps)
        if flips is not None:
            b.set_flips(flips)
        b.decode()
        b.synchronize()
        return [b.download(i) for i in range(len(srcs))], b.path
    finally:
        b.close()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_colour_u8_bit_exact(size):
    """Every operation alone, six mixed programs, the empty program and None, one image each in one batch; a letterbox placement on
    every other image: the fill is part of the image the statistics see."""
    srcs = pick("rgb", len(PROGRAMS))
    pls = [letterbox(size, i) for i in range(len(srcs))]
    outs, path = run(srcs, size, PROGRAMS, "bicubic", pls=pls)
    assert "+place+resize:bicubic" in path and path.endswith("+colour"), path
    changed = 0
    for i, o in enumerate(outs):
        r = resized_u8(srcs[i], size, "bicubic", False, pls[i])
        want = want_u8(r, PROGRAMS[i])
        assert o.size == want.size and np.array_equal(o, want.reshape(-1)), (i, size, PROGRAMS[i], np.nonzero(o != want.reshape(-1))[0][:10].tolist())
        changed += not np.array_equal(want, r)
    assert changed >= 15  # (the programs do something)


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_batch_colour_tensor_with_flips(dtype):
    srcs = pick("rgb", len(MIXED) + 3)
    programs = MIXED + [None, [("equalize", 0)], [("saturation", 0.37), ("contrast", 1.9)]]
    fmt, ref_fmt = TN.fmt_of(dtype)
    flips = [i % 3 != 1 for i in range(len(srcs))]
    for size in ((33, 17), (224, 224)):
        outs, path = run(srcs, size, programs, None, fmt, flips)
        assert path.endswith("+resize+colour+tensor"), path
        for i, o in enumerate(outs):
            u8 = want_u8(resized_u8(srcs[i], size), programs[i], flips[i])
            want = T.bits(T.to_tensor(u8, T.table(ref_fmt, 3), False))
            assert o.shape == (3, size[1], size[0])
            assert np.array_equal(T.bits(o), want), (i, size, programs[i], flips[i], np.argwhere(T.bits(o) != want)[:6].tolist())


@pytest.mark.parametrize("warp", ["nearest", "bilinear"])
def test_colour_before_the_warp_with_a_placement_fill(warp):
    """The placement's fill is recoloured, the warp's is not; u8 and tensor output."""
    size = (33, 17)
    srcs = pick("rgb", len(MIXED) + 2)
    programs = MIXED + [[("invert", 0)], None]
    pls = [letterbox(size, i) for i in range(len(srcs))]
    warps = [None, (1.0, 0.0, 3.3, 0.0, 1.0, -2.7), WR.rotate_matrix(15, size), (1.0, 0.3, -4.0, 0.2, 1.0, 0.0), (-1.0, 0.0, float(size[0]), 0.0, 1.0, 0.0),
             (1.7, 0.0, -5.2, 0.0, 0.9, 3.1), WR.rotate_matrix(90, size), (1.0, 0.0, 5000.0, 0.0, 1.0, 5000.0)]
    outs, path = run(srcs, size, programs, "bicubic", pls=pls, warp=warp, warps=warps)
    assert path.endswith("+colour+warp" + (":bilinear" if warp == "bilinear" else "")), path
    for i, o in enumerate(outs):
        want = want_u8(resized_u8(srcs[i], size, "bicubic", False, pls[i]), programs[i], False, warp, warps[i])
        assert np.array_equal(o, want.reshape(-1)), (i, warp, programs[i], warps[i])
    # (the order matters: an inverted image's warp fill stays the fill)
    r = resized_u8(srcs[6], size, "bicubic", False, pls[6])
    assert not np.array_equal(want_u8(r, programs[6], False, warp, warps[6]), CR.apply(want_u8(r, None, False, warp, warps[6]), programs[6]))
    fmt, ref_fmt = TN.fmt_of("float16")
    flips = [i % 2 == 0 for i in range(len(srcs))]
    outs, path = run(srcs, size, programs, "bicubic", fmt, flips, pls=pls, warp=warp, warps=warps)
    assert path.endswith("+tensor") and "+colour+warp" in path, path
    for i, o in enumerate(outs):
        u8 = want_u8(resized_u8(srcs[i], size, "bicubic", False, pls[i]), programs[i], flips[i], warp, warps[i])
        assert np.array_equal(T.bits(o), T.bits(T.to_tensor(u8, T.table(ref_fmt, 3), False))), (i, warp)


def test_rgb_output_of_gray_and_cmyk_sources_coloured():
    """Gray and CMYK sources give three channels in front of the programs."""
    srcs = sources("other") + sources("rgb")[:2]
    programs = [MIXED[i % len(MIXED)] for i in range(len(srcs))]
    programs[1] = [("saturation", 1.9)]  # (on a gray image: L of three equal channels is the value itself — nothing changes)
    for size in ((33, 17), (224, 224)):
        outs, path = run(srcs, size, programs, None, rgb=True)
        assert "+rgb+resize+colour" in path, path
        for i, o in enumerate(outs):
            want = want_u8(resized_u8(srcs[i], size, None, True), programs[i])
            assert want.shape[2] == 3 and np.array_equal(o, want.reshape(-1)), (i, size, programs[i])


def test_refusals_change_nothing():
    srcs = pick("rgb", 3)
    size = (33, 17)
    good = [MIXED[0], None, MIXED[3]]
    b = batch_of(srcs, size)
    try:
        upload(b, srcs)
        b.set_colour(good)
        for bad in ([("brightness", float("nan"))], [("contrast", float("inf"))], [("saturation", -0.5)], [("brightness", 256.5)], [("solarize", 1.5)],
                    [("solarize", 257)], [("posterize", 0)], [("posterize", 9)], [("posterize", 2.5)], [(9, 0.0)], [("invert", 0)] * 5):
            with pytest.raises(J.FormatError, match="refused"):
                b.set_colour([None, [("invert", 0)], bad])  # (the second program is a good one: it must not stay either)
        with pytest.raises(ValueError):
            b.set_colour([None])
        with pytest.raises(ValueError):
            b.set_colour([[("sharpness", 1.0)], None, None])
        b.decode()
        b.synchronize()
        for i in range(len(srcs)):
            assert np.array_equal(b.download(i), want_u8(resized_u8(srcs[i], size), good[i]).reshape(-1)), i
        with pytest.raises(J.UnsupportedError):
            b.set_warps([None] * 3)  # (matrices are a warped batch's: the identities of the finishing launch are not the caller's)
    finally:
        b.close()
    plain = J.Batch([s["desc"] for s in srcs], output_size=size)
    try:
        with pytest.raises(J.UnsupportedError, match="no colour"):
            plain.set_colour(good)
    finally:
        plain.close()
    with pytest.raises(J.UnsupportedError, match="output size"):
        J.Batch([srcs[0]["desc"]], colour=True)
    co = J._native.ColourOptionsStruct(1)
    hnd = C.c_void_p()
    arr = (J._native.ImageDesc * 1)(srcs[0]["desc"])
    assert J.lib().jpgpu_batch_create_coloured(0, arr, None, None, None, 8, 8, None, None, None, C.byref(co), 1, 0, C.byref(hnd)) == J._native.ERR_FORMAT
    J.lib().jpgpu_batch_destroy(hnd)
    # one and four output channels: the empty program alone
    others = sources("other")[:3]
    b = batch_of(others + srcs[:1], size)
    try:
        upload(b, others + srcs[:1])
        for k in range(3):
            programs = [None] * 4
            programs[k] = [("invert", 0)]
            with pytest.raises(J.UnsupportedError, match="three output channels"):
                b.set_colour(programs)
        b.set_colour([None, [], None, MIXED[1]])
        b.decode()
        b.synchronize()
        for i, s in enumerate(others):
            assert np.array_equal(b.download(i), resized_u8(s, size).reshape(-1)), i
        assert np.array_equal(b.download(3), want_u8(resized_u8(srcs[0], size), MIXED[1]).reshape(-1))
    finally:
        b.close()


def test_no_colour_is_the_batch_without_the_argument():
    """colour=None, and jpgpu_batch_create_coloured without options: the parent's path string and bytes."""
    srcs = pick("rgb", 3)
    size = (33, 17)
    pls = [(22, 15, 5, 1), None, (40, 30, -3, -4)]
    fmt, _ref = TN.fmt_of("float16")
    for tensor in (None, fmt):
        ref = J.Batch([s["desc"] for s in srcs], output_size=size, tensor=tensor, placements=pls, fill=PFILL, filter="bicubic")
        same = batch_of(srcs, size, "bicubic", tensor, pls=pls, colour=None)
        hnd = C.c_void_p()
        arr = (J._native.ImageDesc * len(srcs))(*[s["desc"] for s in srcs])
        ts = tensor.struct() if tensor is not None else None
        st = J.lib().jpgpu_batch_create_coloured(0, arr, None, J.batch.placement_structs(pls, len(srcs)), (C.c_uint8 * 4)(*PFILL), size[0], size[1],
                                                 C.byref(ts) if ts is not None else None, None, None, None, len(srcs), J._native.BATCH_FILTER(3), C.byref(hnd))
        assert st == 0
        try:
            for b in (ref, same):
                upload(b, srcs)
                b.decode()
                b.synchronize()
            assert same.path == ref.path == J.lib().jpgpu_batch_path(hnd).decode() and "colour" not in ref.path and "warp" not in ref.path
            with pytest.raises(J.UnsupportedError):
                same.set_colour(None)
            for i, s in enumerate(srcs):
                for c, a in enumerate(s["coefs"]):
                    a = np.ascontiguousarray(a, np.int16)
                    assert J.lib().jpgpu_batch_upload(hnd, i, c, a.ctypes.data, a.size) == 0
            assert J.lib().jpgpu_batch_decode(hnd, None) == 0 and J.lib().jpgpu_batch_synchronize(hnd, None) == 0
            for i in range(len(srcs)):
                want = ref.download(i)
                assert np.array_equal(same.download(i), want), (i, tensor)
                out = np.empty(want.nbytes, np.uint8)
                got = C.c_size_t(0)
                assert J.lib().jpgpu_batch_download(hnd, i, out.ctypes.data, out.size, C.byref(got)) == 0 and got.value == want.nbytes
                assert np.array_equal(out, want.reshape(-1).view(np.uint8)), (i, tensor)
        finally:
            J.lib().jpgpu_batch_destroy(hnd)
            ref.close()
            same.close()


def test_empty_programs_are_the_batch_without_colour():
    """Every image starts with the empty program: a coloured batch nobody set a program on gives R itself."""
    srcs = pick("rgb", 3) + sources("other")[:1]
    for size in ((224, 224), (33, 17)):
        b = batch_of(srcs, size, "bicubic")
        try:
            upload(b, srcs)
            b.decode()
            b.synchronize()
            for i, s in enumerate(srcs):
                assert np.array_equal(b.download(i), resized_u8(s, size, "bicubic").reshape(-1)), (size, i)
        finally:
            b.close()


def test_new_programs_on_a_kept_batch():
    srcs = pick("rgb", 4)
    size = (33, 17)
    b = batch_of(srcs, size)
    try:
        upload(b, srcs)
        for programs in ([MIXED[0], MIXED[1], None, ALONE[0]], [None, MIXED[5], MIXED[2], MIXED[4]], None):
            b.set_colour(programs)
            b.decode()
            b.synchronize()
            for i in range(len(srcs)):
                assert np.array_equal(b.download(i), want_u8(resized_u8(srcs[i], size), programs[i] if programs else None).reshape(-1)), (programs, i)
    finally:
        b.close()


def test_set_colour_behind_a_pending_decode_on_a_nonblocking_stream():
    """decode; set_colour while that decode is still queued behind torch kernels; decode.  The earlier decode keeps its programs."""
    srcs = pick("rgb", 4)
    size = (33, 17)
    p1, p2 = MIXED[:4], [MIXED[4], None, MIXED[5], [("equalize", 0)]]
    fmt, ref_fmt = TN.fmt_of("float32")
    flips = [False, True, False, True]
    h = StreamHarness("nonblocking")
    b = batch_of(srcs, size, fmt=fmt)
    try:
        upload(b, srcs)
        b.set_flips(flips)
        b.decode(h.handle)  # (the first decode allocates and binds: before the scenario)
        b.synchronize(h.handle)
        snaps = h.buffers(2, b.out_arena_bytes())
        b.set_colour(p1)
        h.ballast()
        b.decode(h.handle)
        ev = h.mark()
        h.snapshot(snaps[0], b.out_arena(), b.out_arena_bytes())
        h.expect_pending(ev, "set_colour")
        b.set_colour(p2)
        h.ballast()
        b.decode(h.handle)
        h.snapshot(snaps[1], b.out_arena(), b.out_arena_bytes())
        h.finish()
        got = snaps.cpu().numpy()
        assert h.checked == 1
        for k, programs in enumerate((p1, p2)):
            for i in range(len(srcs)):
                u8 = want_u8(resized_u8(srcs[i], size), programs[i], flips[i])
                want = T.bits(T.to_tensor(u8, T.table(ref_fmt, 3), False)).reshape(-1)
                o = got[k][b.out_offset(i):b.out_offset(i) + b.out_bytes(i)].view(np.uint32)
                assert np.array_equal(o, want), (k, i)
    finally:
        h.close()
        b.close()


@pytest.mark.parametrize("size", [(33, 17), (224, 224)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_coloured_output_in_a_poisoned_caller_arena(size):
    """A caller's output arena poisoned beforehand: every byte of every image is written, no byte between images changes."""
    hip = RZ._hip()
    srcs = pick("rgb", 5) + sources("other")[:1]
    programs = MIXED[:5] + [None]
    b = batch_of(srcs, size, flags=J._native.BATCH_EXTERNAL_BUFFERS)
    coef, out = C.c_void_p(), C.c_void_p()
    nco, nout = b.coef_arena_bytes(), b.out_arena_bytes()
    assert hip.hipMalloc(C.byref(coef), nco) == 0 and hip.hipMalloc(C.byref(out), nout + 4096) == 0
    try:
        b.bind(coef.value, out.value)
        upload(b, srcs)
        b.set_colour(programs)
        for pattern in (0xA5, 0x3C):
            assert hip.hipMemset(out, pattern, nout + 4096) == 0
            b.decode()
            b.synchronize()
            host = np.empty(nout + 4096, np.uint8)
            assert hip.hipMemcpy(host.ctypes.data, out, nout + 4096, 2) == 0
            covered = np.zeros(nout + 4096, bool)
            for i, s in enumerate(srcs):
                want = want_u8(resized_u8(s, size), programs[i]).reshape(-1)
                off = b.out_offset(i)
                assert b.out_bytes(i) == want.size
                assert np.array_equal(host[off: off + want.size], want), (size, hex(pattern), i)
                covered[off: off + want.size] = True
            assert (host[~covered] == pattern).all(), "the colour stage wrote outside the images"
    finally:
        b.close()
        hip.hipFree(coef)
        hip.hipFree(out)
