"""EXIF orientation in front of the fixed output size (jpgpu_batch_create_oriented, csrc/orient_band.hpp) on the MI355X.  The expected
value is always the references the resize, filter, placement, RGB, tensor and warp tests use, applied to tests/orient_ref.py (the numpy
statement, pinned to Pillow by tests/golden/orient) of the oracle's whole decode, sliced by the window given in ORIENTED coordinates —
compared with np.array_equal."""
import ctypes as C

import numpy as np
import pytest

import filter_ref as F
import orient_ref as OR
import placement_ref as P
import rgb_ref as G
import tensor_ref as T
import test_gpu_filters as FT
import test_gpu_pipeline_windows as PW
import test_gpu_resize as RZ
import test_gpu_tensor as TN
import warp_ref as WR

pytestmark = pytest.mark.gpu

J = None
TILE = 64  # OR_T of csrc/orient_band.hpp
L420, L444, LGRAY, LCMYK = ([(2, 2), (1, 1), (1, 1)], "YCbCr"), ([(1, 1)] * 3, "YCbCr"), ([(1, 1)], "Grayscale"), ([(1, 1)] * 4, "CMYK")
PFILL, WFILL = (114, 7, 200, 33), (9, 250, 77, 140)


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


def oriented_source(case, full, o, win):
    """O of the image's whole output, sliced by the window (x, y, w, h) of O (None: all of it): (h, w, nc)."""
    a = OR.orient(RZ.source_of(case, full, None), o)
    if win is None:
        return a
    x, y, w, h = win
    assert x + w <= a.shape[1] and y + h <= a.shape[0]
    return np.ascontiguousarray(a[y:y + h, x:x + w])


def decode(cases, ors, size, wins=None, **kw):
    flips, warps = kw.pop("flips", None), kw.pop("warps", None)
    b = J.Batch([RZ._desc(c) for c in cases], windows=wins, output_size=size, orientations=ors, **kw)
    try:
        RZ._upload(b, cases)
        if flips is not None:
            b.set_flips(flips)
        if warps is not None:
            b.set_warps(warps)
        b.decode()
        b.synchronize()
        return [b.download(i) for i in range(len(cases))], b.path
    finally:
        b.close()


def edge_sizes():
    T_ = TILE
    return [(1, 1), (1, 37), (37, 1)] + [(h, w) for h in (T_ - 1, T_, T_ + 1) for w in (T_ - 1, T_, T_ + 1)]


_EDGE = {}


def edge_case(layout):
    """One image of 75 x 71 per layout with the oracle's decode, made once."""
    if layout[1] + str(len(layout[0])) + str(layout[0][0]) not in _EDGE:
        rng = np.random.default_rng(190 + len(layout[0]) + layout[0][0][0])
        case = RZ._case(rng, 75, 71, *layout)
        _EDGE[layout[1] + str(len(layout[0])) + str(layout[0][0])] = (case, RZ._full(case))
    return _EDGE[layout[1] + str(len(layout[0])) + str(layout[0][0])]


@pytest.mark.parametrize("layout", [LGRAY, L444, L420, LCMYK], ids=["gray", "444", "420", "cmyk"])
def test_tile_edges_every_orientation(layout):
    """Source windows of 1 x 1, 1 x 37, 37 x 1 and (T-1, T, T+1)^2 at odd coordinates, under every orientation, in one batch: w * nc is
    no multiple of 4 for most of them, and the window's rows start at every byte phase."""
    case, full = edge_case(layout)
    nc = len(layout[0])
    cases, ors, wins = [], [], []
    for (sh, sw) in edge_sizes():
        for o in range(1, 9):
            ww, wh = (sh, sw) if o >= 5 else (sw, sh)
            ow, oh = OR.oriented_size(o, 75, 71)
            win = (3, 5, ww, wh) if (3 + ww <= ow and 5 + wh <= oh) else (1, 1, ww, wh)
            assert OR.source_window(o, 75, 71, win)[2:] == (sw, sh)
            cases.append(case), ors.append(o), wins.append(win)
    assert any((w[2] * nc) % 4 for w in wins) or nc == 4
    size = (37, 29)
    outs, path = decode(cases, ors, size, wins)
    assert "+orient+resize" in path, path
    for i, out in enumerate(outs):
        want = F.resize(oriented_source(case, full, ors[i], wins[i]), size[0], size[1])
        assert np.array_equal(out, want.reshape(-1)), (i, ors[i], wins[i], np.nonzero(out != want.reshape(-1))[0][:8].tolist())


def _mixed():
    """Six images — 4:2:0, gray, CMYK, 4:4:4 — of different sizes with orientations that are not 1, portrait after the rotation."""
    rng = np.random.default_rng(77)
    cases = [RZ._case(rng, 161, 97, *L420), RZ._case(rng, 97, 61, *LGRAY), RZ._case(rng, 150, 67, *LCMYK), RZ._case(rng, 130, 66, *L444),
             RZ._case(rng, 50, 34, *L420), RZ._case(rng, 129, 65, *LGRAY)]
    return cases, [RZ._full(c) for c in cases], [6, 8, 5, 7, 3, 6]


_MIXED = {}


def mixed():
    if not _MIXED:
        _MIXED["v"] = _mixed()
    return _MIXED["v"]


def grid(case):
    return RZ.grid_of(case[0], case[4], case[5])


def test_tensor_f16_with_flips():
    cases, fulls, ors = mixed()
    fmt, ref_fmt = TN.fmt_of("float16")
    flips = [i % 2 == 0 for i in range(len(cases))]
    size = (48, 40)
    outs, path = decode(cases, ors, size, tensor=fmt, flips=flips)
    assert path.endswith("+orient+resize+tensor"), path
    for i, out in enumerate(outs):
        u8 = F.resize(oriented_source(cases[i], fulls[i], ors[i], None), size[0], size[1])
        assert np.array_equal(T.bits(out), T.bits(T.to_tensor(u8, T.table(ref_fmt, u8.shape[2]), flips[i]))), (i, ors[i])


def test_rgb_output_on_gray_and_cmyk():
    cases, fulls, ors = mixed()
    size = (33, 41)
    wins = []
    for c, o in zip(cases, ors):
        ow, oh = OR.oriented_size(o, *grid(c))
        wins.append((1, 3, ow - 2, oh - 5))
    outs, path = decode(cases, ors, size, wins, rgb=True)
    assert "+orient+rgb+resize" in path, path
    for i, out in enumerate(outs):
        want = F.resize(G.to_rgb(oriented_source(cases[i], fulls[i], ors[i], wins[i])), size[0], size[1])
        assert out.size == size[0] * size[1] * 3 and np.array_equal(out, want.reshape(-1)), (i, ors[i])


@pytest.mark.parametrize("mode", ["shorter_side_crop", "letterbox"])
def test_fits_take_the_oriented_size(mode):
    """Landscape files that are portrait after the rotation: the placement comes from the ORIENTED size, and differs from the one the
    file's own size gives."""
    cases, fulls, ors = mixed()
    cases, fulls, ors = cases[:4], fulls[:4], ors[:4]
    size = (40, 40)
    pls, differ = [], 0
    for c, o in zip(cases, ors):
        gw, gh = grid(c)
        ow, oh = OR.oriented_size(o, gw, gh)
        assert oh > ow
        fit = (lambda w, h: P.fit_shorter_side_crop(w, h, 40, *size)) if mode == "shorter_side_crop" else (lambda w, h: P.fit_letterbox(w, h, *size))
        pls.append(tuple(fit(ow, oh)))
        assert pls[-1] == J.fit_placement(J.Fit(mode, 40, PFILL), (ow, oh), size)
        differ += pls[-1] != tuple(fit(gw, gh))
    assert differ == len(cases)
    outs, path = decode(cases, ors, size, placements=pls, fill=PFILL)
    assert "+orient+place+resize" in path, path
    for i, out in enumerate(outs):
        want = F.placed(oriented_source(cases[i], fulls[i], ors[i], None), *pls[i], size[0], size[1], PFILL)
        assert np.array_equal(out, want.reshape(-1)), (i, ors[i], pls[i])


def test_bicubic_on_the_run_route():
    """A CMYK source of 1080 x 64 that orientation 6 turns into 64 x 1080: the resample of the oriented image takes the runs of bands."""
    case, full = FT.block_case("cmyk444", 1080, 64, 1, 2)
    size = (224, 225)
    wins = [(3, 5, 55, 1071), None]
    ors = [6, 8]
    outs, path = decode([case] * 2, ors, size, wins, filter="bicubic", rgb=True)
    assert "+orient+rgb+resize:bicubic+roll" in path, path
    for i, out in enumerate(outs):
        want = F.resize(G.to_rgb(oriented_source(case, full, ors[i], wins[i])), size[0], size[1], F.NAMES["bicubic"])
        assert np.array_equal(out, want.reshape(-1)), (i, np.nonzero(out != want.reshape(-1))[0][:8].tolist())


def test_bilinear_warp_behind_an_oriented_image():
    cases, fulls, ors = mixed()
    size = (33, 21)
    warps = [WR.rotate_matrix(15, size), (1.0, 0.3, -4.0, 0.2, 1.0, 0.0), None, (1.7, 0.0, -5.2, 0.0, 0.9, 3.1), WR.rotate_matrix(90, size), (1.0, 0.0, 3.3, 0.0, 1.0, -2.7)]
    outs, path = decode(cases, ors, size, warp=J.WarpOptions("bilinear", WFILL), warps=warps)
    assert "+orient+resize+warp:bilinear" in path, path
    for i, out in enumerate(outs):
        r = F.resize(oriented_source(cases[i], fulls[i], ors[i], None), size[0], size[1])
        want = WR.warp(r, WR.IDENTITY if warps[i] is None else warps[i], WR.BILINEAR, WFILL)
        assert np.array_equal(out, want.reshape(-1)), (i, ors[i])


@pytest.mark.parametrize("scale", [4, 2, 1])
def test_reduced_size_decodes(scale):
    rng = np.random.default_rng(scale)
    cases = [RZ._case(rng, 250, 130, *L420, scale), RZ._case(rng, 161, 97, *LGRAY, scale), RZ._case(rng, 150, 67, *LCMYK, scale)]
    fulls = [RZ._full(c) for c in cases]
    ors = [6, 7, 4]
    wins = [None, None, None]
    gw, gh = OR.oriented_size(7, *grid(cases[1]))
    if gw > 3 and gh > 3:
        wins[1] = (1, 1, gw - 2, gh - 3)
    size = (31, 45)
    outs, path = decode(cases, ors, size, wins)
    plain = J.Batch([RZ._desc(c) for c in cases], output_size=size)
    base = plain.path
    plain.close()
    assert path == base.replace("+resize", "+orient+resize") or wins[1] is not None, (path, base)  # (the routes stay)
    for i, out in enumerate(outs):
        want = F.resize(oriented_source(cases[i], fulls[i], ors[i], wins[i]), size[0], size[1])
        assert np.array_equal(out, want.reshape(-1)), (i, scale, ors[i])


def test_unwindowed_420_keeps_its_route():
    """Unwindowed 4:2:0 images keep the fused plan (and with it the entry-list walk): only "+orient" is new in the path.  A window
    that covers the oriented image is no window either."""
    rng = np.random.default_rng(420)
    cases = [RZ._case(rng, 161, 97, *L420), RZ._case(rng, 161, 97, *L420)]
    fulls = [RZ._full(c) for c in cases]
    size = (56, 72)
    plain = J.Batch([RZ._desc(c) for c in cases], output_size=size)
    base = plain.path
    plain.close()
    assert "420" in base and base.endswith("+resize"), base
    gw, gh = grid(cases[0])
    for wins in (None, [(0, 0, gh, gw), None]):
        outs, path = decode(cases, [6, 3], size, wins)
        assert path == base.replace("+resize", "+orient+resize"), (path, base)
        for i, out in enumerate(outs):
            want = F.resize(oriented_source(cases[i], fulls[i], [6, 3][i], None), size[0], size[1])
            assert np.array_equal(out, want.reshape(-1)), i


def test_a_batch_mixing_upright_and_oriented_images():
    cases, fulls, _ors = mixed()
    ors = [1, 6, 1, 8, 2, 1]
    size = (48, 40)
    wins = [(3, 1, 90, 60), None, None, (5, 7, 40, 99), None, (0, 0, 129, 65)]
    outs, path = decode(cases, ors, size, wins)
    assert "+orient+resize" in path
    for i, out in enumerate(outs):
        want = F.resize(oriented_source(cases[i], fulls[i], ors[i], wins[i]), size[0], size[1])
        assert np.array_equal(out, want.reshape(-1)), (i, ors[i])


def test_all_ones_is_the_call_without_the_argument():
    cases, fulls, _ors = mixed()
    size = (48, 40)
    wins = [(3, 1, 90, 60), None, None, (5, 7, 99, 40), None, None]
    fmt, _ref = TN.fmt_of("float32")
    for kw in ({}, {"tensor": fmt}, {"rgb": True, "filter": "lanczos"}, {"placements": [(30, 50, 2, -3)] * 6, "fill": PFILL}):
        a, pa = decode(cases, None, size, wins, **kw)
        for ors in ([1] * 6, [None] * 6):
            b, pb = decode(cases, ors, size, wins, **kw)
            assert pa == pb and "orient" not in pb, (pa, pb)
            for x, y in zip(a, b):
                assert np.array_equal(T.bits(x) if x.dtype != np.uint8 else x, T.bits(y) if y.dtype != np.uint8 else y)
    want = F.resize(RZ.source_of(cases[0], fulls[0], wins[0]), size[0], size[1])
    assert np.array_equal(decode(cases, [1] * 6, size, wins)[0][0], want.reshape(-1))


def test_callers_arena_poisoned_every_byte_compared():
    hip = TN._hip()
    cases, fulls, ors = mixed()
    size = (37, 29)
    wins = [None, (1, 3, 50, 90), None, None, (1, 1, 47, 31), None]
    wants = [F.resize(oriented_source(c, f, o, w), size[0], size[1]).reshape(-1) for c, f, o, w in zip(cases, fulls, ors, wins)]
    b = J.Batch([RZ._desc(c) for c in cases], flags=J._native.BATCH_EXTERNAL_BUFFERS, windows=wins, output_size=size, orientations=ors)
    coef, out = C.c_void_p(), C.c_void_p()
    nco, nout = b.coef_arena_bytes(), b.out_arena_bytes()
    assert hip.hipMalloc(C.byref(coef), nco) == 0 and hip.hipMalloc(C.byref(out), nout + 4096) == 0
    try:
        b.bind(coef.value, out.value)
        RZ._upload(b, cases)
        for pattern in (0xA5, 0x3C):
            assert hip.hipMemset(out, pattern, nout + 4096) == 0
            b.decode()
            b.synchronize()
            host = np.empty(nout + 4096, np.uint8)
            assert hip.hipMemcpy(host.ctypes.data, out, nout + 4096, 2) == 0
            end = 0
            for i, want in enumerate(wants):
                off = b.out_offset(i)
                assert (host[end:off] == pattern).all(), (i, "gap")
                assert np.array_equal(host[off:off + want.size], want), (hex(pattern), i, ors[i])
                end = off + want.size
            assert (host[end:] == pattern).all(), "a kernel wrote behind the arena"
    finally:
        b.close()
        hip.hipFree(coef)
        hip.hipFree(out)


def test_refusals():
    cases, _fulls, ors = mixed()
    descs = [RZ._desc(c) for c in cases]
    for bad in (0, 9, 255):
        with pytest.raises(J.FormatError, match="orientation"):
            J.Batch(descs, output_size=(8, 8), orientations=[1, 6, bad, 1, 1, 1])
    with pytest.raises(J.UnsupportedError, match="output size"):
        J.Batch(descs, orientations=ors)
    with pytest.raises(J.FormatError):
        J.Batch(descs, orientations=[1, 1, 0, 1, 1, 1])  # (no size either: the value is refused first)
    with pytest.raises(ValueError):
        J.Batch(descs, output_size=(8, 8), orientations=[6])
    planar = RZ._case(np.random.default_rng(1), 64, 48, [(1, 1)] * 3, "None")
    with pytest.raises(J.UnsupportedError, match="planar"):
        J.Batch([RZ._desc(planar)], output_size=(8, 8), orientations=[6])
    # the window is checked against the ORIENTED size: 161 x 97 under orientation 6 is 97 x 161
    gw, gh = grid(cases[0])
    ok = J.Batch(descs[:1], windows=[(0, 0, gh, gw)], output_size=(8, 8), orientations=[6])
    ok.close()
    with pytest.raises(J.FormatError, match="oriented"):
        J.Batch(descs[:1], windows=[(0, 0, gw, gh)], output_size=(8, 8), orientations=[6])
    # all ones without an output size is the call without the argument
    plain = J.Batch(descs, orientations=[1] * 6)
    assert "orient" not in plain.path
    plain.close()
