"""Placements (jpgpu_batch_create_placed, csrc/placed_band.hpp) on the MI355X: every image resampled to a size of its own and laid into
the fixed output size, cropped and filled.  The expected value is always tests/placement_ref.py (the numpy statement of DESIGN.md
§4.14, pinned to Pillow by tests/golden/placement) on the oracle's whole decode, compared with np.array_equal."""
import ctypes as C

import numpy as np
import pytest

import placement_ref as P
import rgb_ref as G
import tensor_ref as T
import test_gpu_pipeline_windows as PW
import test_gpu_resize as RZ
import test_gpu_tensor as TN
from test_window_emulation import grid_of

pytestmark = pytest.mark.gpu

J = None
FILL = (114, 7, 200, 33)


@pytest.fixture(scope="module", autouse=True)
def _load():
    global J
    import jpeg_decoder_amd as pkg
    J = pkg
    PW.J = pkg
    RZ.J = pkg
    TN.J = pkg
    assert J.device_count() >= 1, "no MI355X visible: the HIP path has no CPU fallback"


def placements_for(canvas, src):
    """Six placements for a source of `src` = (w, h) in `canvas`: crop on both axes with odd offsets; pad on both; crop in x with pad in
    y; one visible pixel at a corner; up-scaling x3; none."""
    (cw, ch), (w, h) = canvas, src
    pw, ph = max(1, (2 * cw) // 3), max(1, ch // 2)
    return [(cw + 31, ch + 17, -15, -9), (pw, ph, (cw - pw) // 2, ch - ph), (cw + 21, max(1, ch // 3), -11, ch // 3), (61, 45, cw - 1, -44), (3 * w, 3 * h, -w, -h), None]


def want_u8(case, full, win, canvas, pl, fill=FILL, rgb=False):
    src = RZ.source_of(case, full, win)
    return P.place(G.to_rgb(src) if rgb else src, canvas[0], canvas[1], pl, fill)


def _decode(cases, wins, canvas, pls, fmt=None, flips=None, rgb=False, fill=FILL, stream=None):
    b = J.Batch([RZ._desc(c) for c in cases], windows=wins, output_size=canvas, tensor=fmt, rgb=rgb, placements=pls, fill=fill)
    try:
        RZ._upload(b, cases)
        if flips is not None:
            b.set_flips(flips)
        b.decode(stream)
        b.synchronize(stream)
        return [b.download(i) for i in range(len(cases))], b.path
    finally:
        b.close()


LAYOUTS = [([(2, 2), (1, 1), (1, 1)], "YCbCr"), ([(1, 1), (1, 1), (1, 1)], "YCbCr"), ([(1, 1)], "Grayscale"), ([(1, 1)] * 4, "CMYK"), ([(2, 1), (1, 1), (1, 1)], "YCbCr")]
SIZES = [(17, 9), (161, 97), (50, 34), (24, 1100), (161, 97), (50, 34)]
CANVASES = [(224, 224), (37, 53), (7, 9), (2048, 3)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{'_'.join(f'{h}{v}' for h, v in l[0])}-{l[1]}")
@pytest.mark.parametrize("scale", [8, 2])
def test_batch_placed_bit_exact(layout, scale):
    """One batch per layout, scale and canvas: six images, six different placements (one of them none), one windowed — every job of the
    launch differs."""
    samp, ct = layout
    rng = np.random.default_rng(1000 + scale + len(samp) * 10)
    cases = [RZ._case(rng, w_, h_, samp, ct, scale) for (w_, h_) in SIZES]
    fulls = [RZ._full(c) for c in cases]
    wins = [None] * len(cases)
    W1, H1 = grid_of(cases[1][0], cases[1][4], cases[1][5])
    wins[1] = (W1 // 5 | 1, H1 // 7 | 1, max(1, (W1 // 2) | 1), max(1, (H1 // 2) | 1))
    for canvas in CANVASES:
        pls = []
        for i, (case, full) in enumerate(zip(cases, fulls)):
            s = RZ.source_of(case, full, wins[i])
            pls.append(placements_for(canvas, (s.shape[1], s.shape[0]))[(i + scale) % 6])
        outs, path = _decode(cases, wins, canvas, pls)
        assert "+place+resize" in path, path
        for i, o in enumerate(outs):
            want = want_u8(cases[i], fulls[i], wins[i], canvas, pls[i]).reshape(-1)
            assert o.size == want.size and np.array_equal(o, want), (i, canvas, pls[i], wins[i], np.nonzero(o != want)[0][:10].tolist())


def test_mostly_padding_and_the_chunked_path():
    rng = np.random.default_rng(3)
    a = RZ._case(rng, 161, 97, [(2, 2), (1, 1), (1, 1)], "YCbCr")
    b = RZ._case(rng, 24, 1100, [(1, 1)] * 3, "RGB")
    for cases, canvas, pl in (([a], (16, 200), (5, 8, 6, 150)), ([b], (7, 7), (2, 1, 1, 3)), ([b, a], (2048, 2), (2500, 1, -200, 1))):
        outs, _p = _decode(cases, None, canvas, [pl] * len(cases))
        for case, o in zip(cases, outs):
            assert np.array_equal(o, want_u8(case, RZ._full(case), None, canvas, pl).reshape(-1)), (canvas, pl)


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_batch_placed_tensor(dtype):
    """Four-pixel items (224 x 224) and element-wise items (37 x 53), flips on half of the images: the tensor is the reference's lookup of
    the placed u8 canvas, the flip mirrors the padding too."""
    rng = np.random.default_rng(44)
    layouts = [LAYOUTS[0], LAYOUTS[2], LAYOUTS[3], LAYOUTS[1], LAYOUTS[0], LAYOUTS[4]]
    cases = [RZ._case(rng, w_, h_, samp, ct) for (samp, ct), (w_, h_) in zip(layouts, SIZES)]
    fulls = [RZ._full(c) for c in cases]
    flips = [i % 2 == 1 for i in range(len(cases))]
    fmt, ref_fmt = TN.fmt_of(dtype)
    for canvas in [(224, 224), (37, 53)]:
        pls = [placements_for(canvas, (c[4], c[5]))[(i + 1) % 6] for i, c in enumerate(cases)]
        outs, path = _decode(cases, None, canvas, pls, fmt, flips, fill=(114, 7, 200))
        assert path.endswith("+place+resize+tensor"), path
        for i, o in enumerate(outs):
            u8 = want_u8(cases[i], fulls[i], None, canvas, pls[i], (114, 7, 200, 0))
            want = T.bits(T.to_tensor(u8, T.table(ref_fmt, u8.shape[2]), flips[i]))
            assert o.shape == (u8.shape[2], canvas[1], canvas[0])
            assert np.array_equal(T.bits(o), want), (i, canvas, pls[i], flips[i], np.argwhere(T.bits(o) != want)[:6].tolist())


def test_placed_tensor_chunked_path():
    """resample_placed_tensor_kernel on the chunked path: a 16 x 1200 image resampled to 16 x 1 and laid at (5, 1) into a 24 x 3 canvas.
    The one visible row's support is every source row; the LDS rows of 64 bytes (shift 15 + 48, rounded up to 16) hold 512 of them, so
    the band takes three chunks.  The bands above and below it are fill.  Plain and flipped, float32."""
    rng = np.random.default_rng(5)
    case = RZ._case(rng, 16, 1200, [(1, 1)] * 3, "RGB")
    full = RZ._full(case)
    canvas, pl, flips = (24, 3), (16, 1, 5, 1), [False, True]
    vb, _ = J.resample_coefficients(1200, 1)
    pitch = (((5 * 3) & 15) + 16 * 3 + 15) & ~15
    assert int(vb[0].sum()) - int(vb[0, 0]) > min(32 * 1024 // pitch, 1200)  # (the row's source rows against placed_plan's cap_rows)
    fmt, ref_fmt = TN.fmt_of("float32")
    outs, path = _decode([case, case], None, canvas, [pl, pl], fmt, flips, fill=(114, 7, 200))
    assert path.endswith("+place+resize+tensor"), path
    u8 = want_u8(case, full, None, canvas, pl, (114, 7, 200, 0))
    for o, flip in zip(outs, flips):
        assert np.array_equal(T.bits(o), T.bits(T.to_tensor(u8, T.table(ref_fmt, 3), flip))), flip


def test_rgb_output_with_pad_placements():
    """A gray and a CMYK file padded on both axes: the fill is in RGB order."""
    rng = np.random.default_rng(9)
    cases = [RZ._case(rng, 50, 34, [(1, 1)], "Grayscale"), RZ._case(rng, 161, 97, [(1, 1)] * 4, "CMYK"), RZ._case(rng, 17, 9, [(2, 2), (1, 1), (1, 1)], "YCbCr")]
    fulls = [RZ._full(c) for c in cases]
    canvas = (64, 48)
    pls = [(40, 27, 13, 11), (33, 20, 1, 27), (70, 20, -3, 5)]
    outs, path = _decode(cases, None, canvas, pls, rgb=True)
    assert path.endswith("+rgb+place+resize"), path
    for i, o in enumerate(outs):
        assert np.array_equal(o, want_u8(cases[i], fulls[i], None, canvas, pls[i], rgb=True).reshape(-1)), i
    fmt, ref_fmt = TN.fmt_of("float16")
    outs, _p = _decode(cases, None, canvas, pls, fmt, [True, False, True], rgb=True)
    for i, o in enumerate(outs):
        u8 = want_u8(cases[i], fulls[i], None, canvas, pls[i], rgb=True)
        assert np.array_equal(T.bits(o), T.bits(T.to_tensor(u8, T.table(ref_fmt, 3), i != 1))), i


@pytest.mark.parametrize("canvas", CANVASES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_arena_canary(canvas):
    """A caller's EXTERNAL_BUFFERS arena poisoned with two patterns: every byte of every canvas is written (fill included), no byte
    between the images or behind the arena changes."""
    hip = TN._hip()
    rng = np.random.default_rng(canvas[0])
    cases = [RZ._case(rng, w_, h_, samp, ct) for (samp, ct), (w_, h_) in zip([LAYOUTS[0], LAYOUTS[2], LAYOUTS[3], LAYOUTS[1]], SIZES)]
    fulls = [RZ._full(c) for c in cases]
    pls = [placements_for(canvas, (c[4], c[5]))[i] for i, c in enumerate(cases)]
    wants = [want_u8(c, f, None, canvas, pl).reshape(-1) for c, f, pl in zip(cases, fulls, pls)]
    b = J.Batch([RZ._desc(c) for c in cases], flags=J._native.BATCH_EXTERNAL_BUFFERS, output_size=canvas, placements=pls, fill=FILL)
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
                assert np.array_equal(host[off:off + want.size], want), (hex(pattern), i, pls[i])
                end = off + want.size
            assert (host[end:] == pattern).all(), "the kernel wrote behind the arena"
    finally:
        b.close()
        hip.hipFree(coef)
        hip.hipFree(out)


def test_identity_placements_are_the_resized_call():
    rng = np.random.default_rng(21)
    cases = [RZ._case(rng, 161, 97, [(2, 2), (1, 1), (1, 1)], "YCbCr"), RZ._case(rng, 50, 34, [(1, 1)], "Grayscale")]
    wins = [(10, 5, 133, 77), None]
    fulls = [RZ._full(c) for c in cases]
    plain, path0 = RZ._decode(cases, wins, (224, 224))
    assert path0 == "mixed+resize"  # (a batch created without placements: the path it always had)
    RZ._check(plain, cases, wins, fulls, (224, 224))
    for pls in ([(224, 224, 0, 0), (224, 224, 0, 0)], [None, (224, 224, 0, 0)], [(0, 0, 5, 5), None]):
        outs, path = _decode(cases, wins, (224, 224), pls)
        assert path == path0, path
        for o, w in zip(outs, plain):
            assert np.array_equal(o, w)


def test_second_decode_after_new_coefficients_and_a_caller_stream():
    hip = TN._hip()
    stream = C.c_void_p()
    assert hip.hipStreamCreateWithFlags(C.byref(stream), 1) == 0  # (hipStreamNonBlocking)
    rng = np.random.default_rng(8)
    first = [RZ._case(rng, 50, 34, [(2, 2), (1, 1), (1, 1)], "YCbCr"), RZ._case(rng, 161, 97, [(1, 1)], "Grayscale")]
    second = [RZ._case(rng, 50, 34, [(2, 2), (1, 1), (1, 1)], "YCbCr"), RZ._case(rng, 161, 97, [(1, 1)], "Grayscale")]
    canvas, pls = (37, 53), [(61, 20, -11, 17), (30, 70, 5, -9)]
    b = J.Batch([RZ._desc(c) for c in first], output_size=canvas, placements=pls, fill=FILL)
    try:
        for cases, s in ((first, None), (second, None), (first, stream), (second, stream)):
            for i, (oc, qts, *_r) in enumerate(cases):
                for c in range(len(oc)):
                    b.set_quantization_table(i, c, qts[c])
            RZ._upload(b, cases)
            b.decode(s)
            b.synchronize(s)
            for i, case in enumerate(cases):
                assert np.array_equal(b.download(i), want_u8(case, RZ._full(case), None, canvas, pls[i]).reshape(-1)), (i, s)
    finally:
        b.close()
        hip.hipStreamDestroy(stream)


def test_refusals():
    rng = np.random.default_rng(1)
    colour = RZ._case(rng, 64, 48, [(2, 2), (1, 1), (1, 1)], "YCbCr")
    planar = RZ._case(rng, 64, 48, [(1, 1)] * 3, "None")
    for pl in [(10, 10, 224, 0), (10, 10, -10, 0), (10, 10, 0, 224), (10, 10, 0, -10), (65535, 1, -65535, 0)]:
        with pytest.raises(J.FormatError, match="shows no pixel"):
            J.Batch([RZ._desc(colour)], output_size=(224, 224), placements=[pl])
    J.Batch([RZ._desc(colour)], output_size=(224, 224), placements=[(10, 10, 223, -9)]).close()
    with pytest.raises(J.UnsupportedError, match="planar"):
        J.Batch([RZ._desc(colour), RZ._desc(planar)], output_size=(8, 8), placements=[(9, 9, 0, 0), None])
    with pytest.raises(ValueError, match="placements"):
        J.Batch([RZ._desc(colour)], output_size=(8, 8), placements=[None, None])
    with pytest.raises(J.FormatError):
        J.Batch([RZ._desc(colour)], placements=[(9, 9, 0, 0)])  # (no output size)
