"""Affine warps (jpgpu_batch_create_warped, csrc/warp_band.hpp) on the MI355X: every image's u8 result of the fixed output size read
through six coefficients of its own.  The expected value is always tests/warp_ref.py (the numpy statement of DESIGN.md §4.16, pinned to
Pillow by tests/golden/warp) applied to the reference result the resize, filter, placement and RGB tests use — tests/filter_ref.py on
the oracle's whole decode —, compared with np.array_equal."""
import ctypes as C

import numpy as np
import pytest

import filter_ref as F
import rgb_ref as G
import tensor_ref as T
import test_gpu_filters as FT
import test_gpu_pipeline_windows as PW
import test_gpu_resize as RZ
import test_gpu_tensor as TN
import warp_ref as WR
from stream_harness import StreamHarness

pytestmark = pytest.mark.gpu

J = None
PFILL, WFILL = (114, 7, 200, 33), (9, 250, 77, 140)
L420, LGRAY, LCMYK = ([(2, 2), (1, 1), (1, 1)], "YCbCr"), ([(1, 1)], "Grayscale"), ([(1, 1)] * 4, "CMYK")
SIZES = [(1, 1), (33, 21), (224, 224)]


@pytest.fixture(scope="module", autouse=True)
def _load():
    global J
    import jpeg_decoder_amd as pkg
    J = pkg
    PW.J = pkg
    RZ.J = pkg
    TN.J = pkg
    FT.J = pkg
    assert J.device_count() >= 1, "no MI355X visible: the HIP path has no CPU fallback"


def matrices(size):
    """The matrix kinds of tests/golden/warp for an output of `size`: identity, fractional translation, pure scale, negative m[0], a quarter
    turn, a rotation, a shear, everything outside, a large zoom, a translation at the refusal bound."""
    w, h = size
    return [None, (1.0, 0.0, 3.3, 0.0, 1.0, -2.7), (1.7, 0.0, -5.2, 0.0, 0.9, 3.1), (-1.0, 0.0, float(w), 0.0, 1.0, 0.0), WR.rotate_matrix(90, size),
            WR.rotate_matrix(15, size), (1.0, 0.3, -4.0, 0.2, 1.0, 0.0), (1.0, 0.0, 5000.0, 0.0, 1.0, 5000.0), (0.01, 0.002, w / 3.0, -0.003, 0.01, h / 2.0),
            (1.0, 0.0, 32000.0 - w, 0.0, 1.0, -32000.0)]


_SOURCES = {}


def sources():
    """Ten sources of about 48 x 40 — gray, 4:2:0 and CMYK in turn — with the oracle's decode, made once."""
    if not _SOURCES:
        rng = np.random.default_rng(416)
        cases = [RZ._case(rng, 48 + (i % 3), 40 - (i % 2), *[LGRAY, L420, LCMYK][i % 3]) for i in range(10)]
        _SOURCES["cases"], _SOURCES["fulls"] = cases, [RZ._full(c) for c in cases]
    return _SOURCES["cases"], _SOURCES["fulls"]


def letterbox(size, i):
    """A placement that pads (both fills show) for every other image."""
    w, h = size
    return None if (i % 2 or w < 4 or h < 4) else (max(1, (2 * w) // 3), max(1, h - 2), w // 6, 1)


def resized_u8(case, full, size, name, rgb, pl):
    """R: the image's u8 result without a warp."""
    src = RZ.source_of(case, full, None)
    src = G.to_rgb(src) if rgb else src
    f = F.NAMES[name or "bilinear"]
    return F.resize(src, size[0], size[1], f) if pl is None else F.placed(src, *pl, size[0], size[1], PFILL, f)


def want_of(r, m, filt, flip=False):
    return WR.warp(r[:, ::-1] if flip else r, WR.IDENTITY if m is None else m, WR.BILINEAR if filt == "bilinear" else WR.NEAREST, WFILL)


def batch_of(cases, size, filt, name=None, fmt=None, rgb=False, pls=None, flags=0):
    return J.Batch([RZ._desc(c) for c in cases], flags=flags, output_size=size, tensor=fmt, rgb=rgb, placements=pls, fill=PFILL, filter=name,
                   warp=J.WarpOptions(filt, WFILL))


def run(cases, size, filt, warps, name=None, fmt=None, flips=None, rgb=False, pls=None):
    b = batch_of(cases, size, filt, name, fmt, rgb, pls)
    try:
        RZ._upload(b, cases)
        b.set_warps(warps)
        if flips is not None:
            b.set_flips(flips)
        b.decode()
        b.synchronize()
        return [b.download(i) for i in range(len(cases))], b.path
    finally:
        b.close()


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
def test_batch_warp_u8_bit_exact(filt, size):
    """Ten images, ten matrix kinds in one batch, a bicubic resample in front, a letterbox placement on every other image."""
    cases, fulls = sources()
    warps = matrices(size)
    pls = [letterbox(size, i) for i in range(len(cases))]
    outs, path = run(cases, size, filt, warps, "bicubic", pls=pls)
    assert ("+place+resize:bicubic" in path or size[0] < 4) and path.endswith("+warp:bilinear" if filt == "bilinear" else "+warp"), path
    changed = 0
    for i, o in enumerate(outs):
        r = resized_u8(cases[i], fulls[i], size, "bicubic", False, pls[i])
        want = want_of(r, warps[i], filt)
        assert o.size == want.size and np.array_equal(o, want.reshape(-1)), (i, size, warps[i], np.nonzero(o != want.reshape(-1))[0][:10].tolist())
        changed += not np.array_equal(want, r)
    assert changed >= (5 if size != (1, 1) else 1)  # (the matrices do something)


@pytest.mark.parametrize("dtype", ["float32", "float16", "bfloat16"])
def test_batch_warp_tensor_with_flips(dtype):
    """The flip comes before the warp; an element outside the source is T[c][wfill[c]]."""
    cases, fulls = sources()
    fmt, ref_fmt = TN.fmt_of(dtype)
    flips = [i % 3 != 1 for i in range(len(cases))]
    for size, filt in (((33, 21), "bilinear"), ((224, 224), "nearest"), ((33, 21), "nearest"), ((1, 1), "bilinear")):
        warps = matrices(size)
        pls = [letterbox(size, i) for i in range(len(cases))]
        outs, path = run(cases, size, filt, warps, "bicubic", fmt, flips, pls=pls)
        assert path.endswith(("+warp:bilinear" if filt == "bilinear" else "+warp") + "+tensor"), path
        for i, o in enumerate(outs):
            r = resized_u8(cases[i], fulls[i], size, "bicubic", False, pls[i])
            u8 = want_of(r, warps[i], filt, flips[i])
            want = T.bits(T.to_tensor(u8, T.table(ref_fmt, u8.shape[2]), False))
            assert o.shape == (u8.shape[2], size[1], size[0])
            assert np.array_equal(T.bits(o), want), (i, size, filt, warps[i], flips[i], np.argwhere(T.bits(o) != want)[:6].tolist())
        if size == (33, 21):  # (the order matters: warping first and mirroring afterwards gives another image)
            r = resized_u8(cases[5], fulls[5], size, "bicubic", False, pls[5])
            assert flips[5] and not np.array_equal(want_of(r, warps[5], filt, True), want_of(r, warps[5], filt)[:, ::-1])


def test_rgb_output_warped():
    """Gray and CMYK sources give three channels before the warp: the warp's fill is in RGB order."""
    cases, fulls = sources()
    size = (33, 21)
    warps = matrices(size)[::-1]
    pls = [letterbox(size, i + 1) for i in range(len(cases))]
    for filt in ("nearest", "bilinear"):
        outs, path = run(cases, size, filt, warps, None, rgb=True, pls=pls)
        assert "+rgb+place+resize+warp" in path, path
        for i, o in enumerate(outs):
            want = want_of(resized_u8(cases[i], fulls[i], size, None, True, pls[i]), warps[i], filt)
            assert np.array_equal(o, want.reshape(-1)), (i, filt, warps[i])
    fmt, ref_fmt = TN.fmt_of("float16")
    flips = [i % 2 == 0 for i in range(len(cases))]
    outs, _p = run(cases, size, "bilinear", warps, None, fmt, flips, rgb=True, pls=pls)
    for i, o in enumerate(outs):
        u8 = want_of(resized_u8(cases[i], fulls[i], size, None, True, pls[i]), warps[i], "bilinear", flips[i])
        assert np.array_equal(T.bits(o), T.bits(T.to_tensor(u8, T.table(ref_fmt, 3), False))), i


@pytest.mark.parametrize("filt", ["nearest", "bilinear"])
def test_warp_behind_a_window_and_a_run_route(filt):
    """The CMYK 64 x 1080 source of test_gpu_filters.test_cmyk_on_the_run_route, windowed at odd coordinates, under RGB output to
    (224, 225): the run route in front of a rotation and a shear (rule N under NEAREST, rule B under BILINEAR).  `+roll` stands in
    front of `+warp` in the path."""
    size = (224, 225)
    case, full = FT.block_case("cmyk444", 64, 1080, 2, 1)
    wins = [(5, 3, 55, 1071), (1, 7, 61, 1069)]
    warps = [WR.rotate_matrix(15, size), (1.0, 0.3, -4.0, 0.2, 1.0, 0.0)]
    assert all(m[1] != 0.0 and m[3] != 0.0 for m in warps)  # (not the N-sep tables)
    fmt, ref_fmt = TN.fmt_of("float16")
    flips = [True, False]
    for name in FT.WIDE:
        for tensor in (None, fmt):
            b = J.Batch([RZ._desc(case)] * 2, windows=wins, output_size=size, tensor=tensor, rgb=True, filter=name, warp=J.WarpOptions(filt, WFILL))
            try:
                RZ._upload(b, [case] * 2)
                b.set_warps(warps)
                if tensor is not None:
                    b.set_flips(flips)
                b.decode()
                b.synchronize()
                outs, path = [b.download(i) for i in range(2)], b.path
            finally:
                b.close()
            assert ("+rgb+resize:" + name + "+roll+warp" + (":bilinear" if filt == "bilinear" else "")) in path and path.endswith("+tensor") == (tensor is not None), path
            for i, o in enumerate(outs):
                r = F.resize(G.to_rgb(RZ.source_of(case, full, wins[i])), size[0], size[1], F.NAMES[name])
                want = want_of(r, warps[i], filt, flips[i] and tensor is not None)
                assert not np.array_equal(want, r)
                if tensor is None:
                    assert np.array_equal(o, want.reshape(-1)), (name, filt, i, np.nonzero(o != want.reshape(-1))[0][:10].tolist())
                else:
                    assert np.array_equal(T.bits(o), T.bits(T.to_tensor(want, T.table(ref_fmt, 3), False))), (name, filt, i)


def _nsep_matrix(w, h):
    """A matrix without rotation or shear whose pixels on a w x h image differ between rule N-sep (Pillow's) and rule N, found on the CPU."""
    rng = np.random.default_rng(2048)
    probe = np.arange(w * h, dtype=np.uint32).reshape(h, w, 1)
    probe = np.concatenate([probe & 255, (probe >> 8) & 255, probe >> 16], axis=2).astype(np.uint8)
    for _ in range(200):
        m = (float(rng.uniform(0.3, 1.2)), 0.0, float(rng.uniform(-300, 50)), 0.0, float(rng.uniform(0.5, 1.5)), float(rng.uniform(-1, 1)))
        if not np.array_equal(WR.nearest_separable(probe, m), WR.nearest_fixed(probe, m)):
            return m
    raise AssertionError("no N-sep matrix differs from rule N")


def test_nsep_is_not_rule_n_on_a_wide_output():
    rng = np.random.default_rng(64)
    case = RZ._case(rng, 64, 16, *L420)
    size = (2048, 2)
    m = _nsep_matrix(*size)
    outs, _p = run([case], size, "nearest", [m])
    r = resized_u8(case, RZ._full(case), size, None, False, None)
    want = want_of(r, m, "nearest")
    assert not np.array_equal(want, WR.nearest_fixed(r, m, WFILL))  # (the case discriminates on THIS image)
    assert np.array_equal(outs[0], want.reshape(-1)), np.nonzero(outs[0] != want.reshape(-1))[0][:10].tolist()


def test_set_warps_behind_a_pending_decode_on_a_nonblocking_stream():
    """decode; set_warps while that decode is still queued behind torch kernels; decode.  The earlier decode keeps its matrices."""
    cases, fulls = sources()
    cases, fulls = cases[:4], fulls[:4]
    size = (33, 21)
    w1, w2 = matrices(size)[1:5], matrices(size)[5:9]
    fmt, ref_fmt = TN.fmt_of("float32")
    flips = [False, True, False, True]
    h = StreamHarness("nonblocking")
    b = batch_of(cases, size, "bilinear", fmt=fmt)
    try:
        RZ._upload(b, cases)
        b.set_flips(flips)
        b.decode(h.handle)  # (the first decode allocates and binds: before the scenario)
        b.synchronize(h.handle)
        snaps = h.buffers(2, b.out_arena_bytes())
        b.set_warps(w1)
        h.ballast()
        b.decode(h.handle)
        ev = h.mark()
        h.snapshot(snaps[0], b.out_arena(), b.out_arena_bytes())
        h.expect_pending(ev, "set_warps")
        b.set_warps(w2)
        h.ballast()
        b.decode(h.handle)
        h.snapshot(snaps[1], b.out_arena(), b.out_arena_bytes())
        h.finish()
        got = snaps.cpu().numpy()
        assert h.checked == 1
        for k, warps in enumerate((w1, w2)):
            for i in range(len(cases)):
                u8 = want_of(resized_u8(cases[i], fulls[i], size, None, False, None), warps[i], "bilinear", flips[i])
                want = T.bits(T.to_tensor(u8, T.table(ref_fmt, u8.shape[2]), False)).reshape(-1)
                o = got[k][b.out_offset(i):b.out_offset(i) + b.out_bytes(i)].view(np.uint32)
                assert np.array_equal(o, want), (k, i)
    finally:
        h.close()
        b.close()


def test_refusals_change_nothing():
    cases, fulls = sources()
    cases, fulls = cases[:3], fulls[:3]
    size = (33, 21)
    good = matrices(size)[4:7]
    b = batch_of(cases, size, "nearest")
    try:
        RZ._upload(b, cases)
        b.set_warps(good)
        for bad in ((float("nan"), 0, 0, 0, 1, 0), (1, 0, float("inf"), 0, 1, 0), (16000.5, 0, 0, 0, 1, 0), (1, 0, 0, -16001.0, 1, 0), (1, 0, 32000.5, 0, 1, 0),
                    (1, 0, 0, 0, 1, -32001.0), (1000.0, 0, 0, 0, 1, 0)):
            with pytest.raises(J.FormatError, match="refused"):
                b.set_warps([None, (1, 0, 1, 0, 1, 1), bad])  # (the second matrix is a good one: it must not stay either)
        with pytest.raises(ValueError):
            b.set_warps([None])
        b.decode()
        b.synchronize()
        for i in range(len(cases)):
            want = want_of(resized_u8(cases[i], fulls[i], size, None, False, None), good[i], "nearest")
            assert np.array_equal(b.download(i), want.reshape(-1)), i
        with pytest.raises(J.UnsupportedError):
            b.set_flips([True] * 3)  # (flips are a tensor batch's)
    finally:
        b.close()
    plain = J.Batch([RZ._desc(c) for c in cases], output_size=size)
    try:
        with pytest.raises(J.UnsupportedError, match="no warp"):
            plain.set_warps(good)
    finally:
        plain.close()
    planar = RZ._case(np.random.default_rng(1), 64, 48, [(1, 1)] * 3, "None")
    with pytest.raises(J.UnsupportedError, match="planar"):
        J.Batch([RZ._desc(planar)], output_size=size, warp=J.WarpOptions())
    with pytest.raises(J.FormatError, match="output size"):
        J.Batch([RZ._desc(cases[0])], warp=J.WarpOptions())
    wo = J._native.WarpOptionsStruct()
    for filt, reserved in ((2, 0), (0, 1)):
        wo.filter, wo.reserved = filt, reserved
        hnd = C.c_void_p()
        arr = (J._native.ImageDesc * 1)(RZ._desc(cases[0]))
        st = J.lib().jpgpu_batch_create_warped(0, arr, None, None, None, 8, 8, None, C.byref(wo), 1, 0, C.byref(hnd))
        assert st == J._native.ERR_FORMAT
        J.lib().jpgpu_batch_destroy(hnd)
    with pytest.raises(ValueError):
        J.WarpOptions("bicubic")


def test_null_options_are_the_placed_call():
    """jpgpu_batch_create_warped without options: the parent's path string and bytes."""
    cases, fulls = sources()
    cases = cases[:3]
    size = (33, 21)
    pls = [(22, 19, 5, 1), None, (40, 30, -3, -4)]
    fmt, _ref = TN.fmt_of("float16")
    for tensor in (None, fmt):
        ref = J.Batch([RZ._desc(c) for c in cases], output_size=size, tensor=tensor, placements=pls, fill=PFILL, filter="bicubic")
        hnd = C.c_void_p()
        arr = (J._native.ImageDesc * len(cases))(*[RZ._desc(c) for c in cases])
        ts = tensor.struct() if tensor is not None else None
        st = J.lib().jpgpu_batch_create_warped(0, arr, None, J.batch.placement_structs(pls, len(cases)), (C.c_uint8 * 4)(*PFILL), size[0], size[1],
                                               C.byref(ts) if ts is not None else None, None, len(cases), J._native.BATCH_FILTER(3), C.byref(hnd))
        assert st == 0
        try:
            RZ._upload(ref, cases)
            ref.decode()
            ref.synchronize()
            assert J.lib().jpgpu_batch_path(hnd).decode() == ref.path and "warp" not in ref.path
            for i, (oc, _q, coefs, *_r) in enumerate(cases):
                for c in range(len(oc)):
                    a = np.ascontiguousarray(coefs[c], np.int16)
                    assert J.lib().jpgpu_batch_upload(hnd, i, c, a.ctypes.data, a.size) == 0
            assert J.lib().jpgpu_batch_decode(hnd, None) == 0 and J.lib().jpgpu_batch_synchronize(hnd, None) == 0
            for i in range(len(cases)):
                want = ref.download(i)
                out = np.empty(want.nbytes, np.uint8)
                got = C.c_size_t(0)
                assert J.lib().jpgpu_batch_download(hnd, i, out.ctypes.data, out.size, C.byref(got)) == 0 and got.value == want.nbytes
                assert np.array_equal(out, want.reshape(-1).view(np.uint8)), (i, tensor)
        finally:
            J.lib().jpgpu_batch_destroy(hnd)
            ref.close()


def test_identity_warp_is_the_batch_without_a_warp():
    """Every image starts with the identity: a warped batch nobody set a matrix on gives R itself, under both filters."""
    cases, fulls = sources()
    size = (224, 224)
    for filt in ("nearest", "bilinear"):
        outs, _p = run(cases[:3], size, filt, None, "bicubic")
        for i, o in enumerate(outs):
            assert np.array_equal(o, resized_u8(cases[i], fulls[i], size, "bicubic", False, None).reshape(-1)), (filt, i)
