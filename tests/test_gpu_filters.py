"""The resample filters (JPGPU_BATCH_FILTER) on the MI355X: BOX, HAMMING, BICUBIC and LANCZOS through every route to a
fixed output size.  The expected value is always tests/filter_ref.py (the numpy statement, pinned to Pillow by tests/golden/filters)
applied to the oracle's whole decode, sliced, compared with np.array_equal.  The sources are high-contrast — 0 / 255 block patterns at
quantization tables of ones (q100) — and the tests assert on the CPU that the reference's unclamped sums fall below 0 and above
255 * 2^22 in BOTH passes: otherwise the clamps the negative weights need would not be tested."""
import numpy as np
import pytest

import filter_ref as F
import oracle as O
import placement_ref as P
import rgb_ref as G
import tensor_ref as T
import test_gpu_pipeline_windows as PW
import test_gpu_resize as RZ
import test_gpu_tensor as TN

pytestmark = pytest.mark.gpu

J = None
NEW = ["box", "hamming", "bicubic", "lanczos"]
WIDE = ["bicubic", "lanczos"]
ONE = 255 << 22
LDS = 32 * 1024  # RS_MAX_LDS


@pytest.fixture(scope="module", autouse=True)
def _load():
    global J
    import jpeg_decoder_amd as pkg
    J = pkg
    PW.J = pkg
    RZ.J = pkg
    TN.J = pkg
    assert J.device_count() >= 1, "no MI355X visible: the HIP path has no CPU fallback"


LAYOUTS = {"420": ([(2, 2), (1, 1), (1, 1)], "YCbCr"), "gray": ([(1, 1)], "Grayscale"), "cmyk444": ([(1, 1)] * 4, "CMYK"), "444": ([(1, 1)] * 3, "YCbCr")}
_CASES = {}


def block_case(layout, w_, h_, by=1, bx=1, seed=0):
    """An image of 0 / 255 blocks: DC-only coefficients of +-1024 under tables of ones, constant over by x bx blocks of each component
    (8 by x 8 bx pixels of luma).  Cached with the oracle's decode: -> (case, full)."""
    key = (layout, w_, h_, by, bx, seed)
    if key not in _CASES:
        samp, ct = LAYOUTS[layout]
        rng = np.random.default_rng(seed * 7919 + w_ * 31 + h_)
        ocomps, _ = O.make_components(w_, h_, samp)
        qts = [np.ones(64, np.uint16) for _ in ocomps]
        coefs = []
        for c in ocomps:
            bw, bh = int(c.block_w), int(c.block_h)
            sign = rng.integers(0, 2, (-(-bh // by), -(-bw // bx))).repeat(by, axis=0).repeat(bx, axis=1)[:bh, :bw]
            a = np.zeros((bh, bw, 64), np.int16)
            a[:, :, 0] = np.where(sign == 1, 1024, -1024)
            coefs.append(a.reshape(-1))
        case = (ocomps, qts, coefs, ct, w_, h_)
        full = RZ._full(case)
        assert np.isin(full, (0, 255)).mean() >= (0.4 if ct == "YCbCr" else 1.0)  # (chroma at its extremes moves some colours inside)
        _CASES[key] = (case, full)
    return _CASES[key]


def want_u8(f, case, full, win, size, rgb=False, pl=None, fill=(0, 0, 0, 0), sums=None):
    src = RZ.source_of(case, full, win)
    src = G.to_rgb(src) if rgb else src
    if pl is None:
        return F.resize(src, size[0], size[1], f, sums=sums)
    return F.placed(src, *pl, size[0], size[1], fill, f)


def ends(path, suffix):
    """The path ends in `suffix`; where some image's plan takes the run route, `+roll` follows."""
    return path.endswith(suffix) or path.endswith(suffix + "+roll")


def clamps_at_both_ends(sums):
    """The unclamped sums of the horizontal AND of the vertical pass leave 0..255 on both sides."""
    return len(sums) == 2 and all(lo < 0 and hi >= ONE + (1 << 22) for lo, hi in sums)


def decode(cases, wins, size, name, fmt=None, flips=None, rgb=False, pls=None, fill=None):
    b = J.Batch([RZ._desc(c) for c in cases], windows=wins, output_size=size, tensor=fmt, rgb=rgb, placements=pls, fill=fill, filter=name)
    try:
        RZ._upload(b, cases)
        if flips is not None:
            b.set_flips(flips)
        b.decode()
        b.synchronize()
        return [b.download(i) for i in range(len(cases))], b.path
    finally:
        b.close()


def plan_of(name, in_h, out_w, out_h, nc):
    """resample_plan restated on the library's own tables: (rb, bands, cap_rows, [(s0, s1) per band])."""
    vb, _ = J.resample_coefficients(in_h, out_h, name)
    pitch = (out_w * nc + 3) & ~3
    cap = min(LDS // pitch, in_h)

    def spans(rb):
        return [(int(vb[r0, 0]), int(vb[min(r0 + rb, out_h) - 1].sum())) for r0 in range(0, out_h, rb)]

    rb = min(64, out_h)
    while rb > 1 and any(s1 - s0 > cap for s0, s1 in spans(rb)):
        rb -= 1
    return rb, -(-out_h // rb), cap, spans(rb)


@pytest.mark.parametrize("layout", ["420", "gray", "cmyk444"])
@pytest.mark.parametrize("name", NEW)
def test_batch_filter_bit_exact(name, layout):
    """A 97 x 61 image to (37, 53): whole, and windowed at odd coordinates, in one launch."""
    f = F.NAMES[name]
    case, full = block_case(layout, 97, 61)
    wins = [None, (5, 3, 87, 55), (1, 7, 95, 47)]
    outs, path = decode([case] * 3, wins, (37, 53), name)
    assert ends(path, "+resize:" + name), path
    for i, (o, win) in enumerate(zip(outs, wins)):
        sums = []
        want = want_u8(f, case, full, win, (37, 53), sums=sums)
        if name in WIDE:
            assert clamps_at_both_ends(sums), (i, sums)  # (else the clamps are not tested)
        assert np.array_equal(o, want.reshape(-1)), (name, layout, win, np.nonzero(o != want.reshape(-1))[0][:10].tolist())


def test_a_small_window_up_to_a_larger_size_overshoots():
    """A 9 x 7 window up to 64 x 48: at scale < 1 the support stays S_F pixels, the negative lobes overshoot at every edge."""
    case, full = block_case("420", 97, 61)
    win = (11, 5, 9, 7)  # (the block edges at x = 16 and y = 8 cross it)
    for name in NEW:
        sums = []
        want = want_u8(F.NAMES[name], case, full, win, (64, 48), sums=sums)
        if name in WIDE:
            assert clamps_at_both_ends(sums), (name, sums)
        outs, _p = decode([case], [win], (64, 48), name)
        assert np.array_equal(outs[0], want.reshape(-1)), name


def test_an_output_size_equal_to_the_window_is_the_window():
    for layout in ("420", "gray", "cmyk444"):
        case, full = block_case(layout, 97, 61)
        win = (5, 3, 37, 53)
        src = RZ.source_of(case, full, win).reshape(-1)
        for name in NEW:
            outs, _p = decode([case], [win], (37, 53), name)
            assert np.array_equal(outs[0], src), (layout, name)


@pytest.mark.parametrize("name", WIDE)
def test_chunked_path(name):
    """A 16 x 1200 image to (16, 1): the row's support is every source row and takes two chunks of 682 three-channel rows (three of 512
    CMYK rows).  With one output row the filter's argument stays within (-0.5, 0.5) and every weight is positive; (16, 3) beside it
    reaches the negative lobes, so that a chunk's partial sum can be negative."""
    f = F.NAMES[name]
    for layout, nc in (("444", 3), ("cmyk444", 4)):
        case, full = block_case(layout, 16, 1200, 19, 1)
        for oh in (1, 3):
            rb, bands, cap, spans = plan_of(name, 1200, 16, oh, nc)
            assert rb == 1 and max(s1 - s0 for s0, s1 in spans) > cap, (rb, cap, spans)
            _, vk = J.resample_coefficients(1200, oh, name)
            assert (vk < 0).any() == (oh == 3)
            outs, _p = decode([case], None, (16, oh), name)
            assert np.array_equal(outs[0], want_u8(f, case, full, None, (16, oh)).reshape(-1)), (name, layout, oh)


def test_one_row_per_band_in_one_chunk():
    """Rows so wide that LDS holds four (bicubic: 2048 CMYK pixels) or six (lanczos: 1707 three-channel pixels) of them: one output
    row's support fits, two neighbours' does not — rb == 1 on the one-chunk path."""
    for name, layout, nc, ow in (("bicubic", "cmyk444", 4, 2048), ("lanczos", "444", 3, 1707)):
        case, full = block_case(layout, 24, 40)
        rb, bands, cap, spans = plan_of(name, 40, ow, 40, nc)
        assert rb == 1 and bands == 40 and max(s1 - s0 for s0, s1 in spans) == cap, (name, rb, cap, spans)
        outs, _p = decode([case], None, (ow, 40), name)
        assert np.array_equal(outs[0], want_u8(F.NAMES[name], case, full, None, (ow, 40)).reshape(-1)), name


@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_tensor_with_flips(dtype):
    fmt, ref_fmt = TN.fmt_of(dtype)
    cases = [block_case("420", 97, 61), block_case("gray", 97, 61), block_case("cmyk444", 97, 61), block_case("420", 97, 61, seed=1)]
    wins = [(5, 3, 87, 55), None, (1, 7, 95, 47), None]
    flips = [True, False, True, True]
    for name in NEW:
        for size in ((37, 53), (224, 224)):  # (element-wise items and four-pixel items)
            outs, path = decode([c for c, _f in cases], wins, size, name, fmt, flips)
            assert ends(path, "+resize:" + name + "+tensor"), path
            for i, ((case, full), o) in enumerate(zip(cases, outs)):
                u8 = want_u8(F.NAMES[name], case, full, wins[i], size)
                want = T.bits(T.to_tensor(u8, T.table(ref_fmt, u8.shape[2]), flips[i]))
                assert o.shape == (u8.shape[2], size[1], size[0]) and np.array_equal(T.bits(o), want), (name, size, i)


def test_rgb_output_from_gray_and_cmyk():
    cases = [block_case("gray", 97, 61), block_case("cmyk444", 97, 61), block_case("420", 97, 61)]
    wins = [(5, 3, 87, 55), (4, 7, 91, 47), None]
    fmt, ref_fmt = TN.fmt_of("float16")
    for name in NEW:
        f = F.NAMES[name]
        outs, path = decode([c for c, _f in cases], wins, (37, 53), name, rgb=True)
        assert ends(path, "+rgb+resize:" + name), path
        wants = [want_u8(f, case, full, wins[i], (37, 53), rgb=True) for i, (case, full) in enumerate(cases)]
        for i, o in enumerate(outs):
            assert np.array_equal(o, wants[i].reshape(-1)), (name, i)
        outs, _p = decode([c for c, _f in cases], wins, (37, 53), name, fmt, [False, True, True], rgb=True)
        for i, o in enumerate(outs):
            assert np.array_equal(T.bits(o), T.bits(T.to_tensor(wants[i], T.table(ref_fmt, 3), i != 0))), (name, i)


def test_placements():
    """A letterbox (fill above and below), and a shorter-side crop that lies partly outside the canvas (range tables with first > 0),
    u8 and tensor; a gray image padded on both axes."""
    cases = [block_case("420", 97, 61), block_case("420", 97, 61, seed=1), block_case("gray", 97, 61)]
    size, fill = (48, 48), (114, 7, 200, 33)
    pls = [P.fit_letterbox(97, 61, 48, 48), P.fit_shorter_side_crop(97, 61, 48, 48, 48), (30, 21, 11, 20)]
    assert pls[0][3] > 0 and pls[1][2] < 0 and pls[1][0] > 48
    fmt, ref_fmt = TN.fmt_of("bfloat16")
    for name in NEW:
        f = F.NAMES[name]
        outs, path = decode([c for c, _f in cases], None, size, name, pls=pls, fill=fill)
        assert ends(path, "+place+resize:" + name), path
        wants = [want_u8(f, case, full, None, size, pl=pl, fill=fill) for (case, full), pl in zip(cases, pls)]
        for i, o in enumerate(outs):
            assert np.array_equal(o, wants[i].reshape(-1)), (name, i, pls[i])
        outs, path = decode([c for c, _f in cases], None, size, name, fmt, [True, False, True], pls=pls, fill=fill)
        assert ends(path, "+place+resize:" + name + "+tensor"), path
        for i, o in enumerate(outs):
            want = T.to_tensor(wants[i], T.table(ref_fmt, wants[i].shape[2]), i != 1)
            assert np.array_equal(T.bits(o), T.bits(want)), (name, i, pls[i])


ROLL_MIN, ROLL_LONG = 1.30, 32  # RS_ROLL_MIN_PERCENT, RS_ROLL_LONG_BANDS of csrc/resample_band.hpp: 8 bands per run from 32 bands on, else 4


@pytest.mark.parametrize("name", WIDE)
def test_runs_of_bands(name):
    """A 64 x 1080 source to (224, 225): bands of 7 (bicubic) or 4 (lanczos) output rows whose source rows overlap 1.4 / 2.2 times take
    the run route — at least two runs, at least three bands in a run, a shorter last run (asserted on the plan) — beside an image of
    the same batch that keeps its bands (97 x 61, up-scaled: nothing overlaps enough).  u8 and tensor, bit-exact, `+roll` in the path.
    (The 64 x 400 source to (24, 40) plans ONE band — 400 rows of 72 bytes fit in LDS — so it cannot show a run.)"""
    f = F.NAMES[name]
    size = (224, 225)
    tall, small = block_case("444", 64, 1080, 2, 1), block_case("420", 97, 61)
    rb, bands, cap, spans = plan_of(name, 1080, 224, 225, 3)
    redundancy = sum(s1 - s0 for s0, s1 in spans) / (spans[-1][1] - spans[0][0])
    bpr = 8 if bands >= ROLL_LONG else 4
    runs = -(-bands // bpr)
    assert all(s1 - s0 <= cap for s0, s1 in spans) and redundancy > ROLL_MIN, (rb, bands, redundancy)
    assert runs >= 2 and bpr >= 3 and 0 < bands - (runs - 1) * bpr < bpr, (bands, runs)
    _rb, _bands, _cap, sp = plan_of(name, 61, 224, 225, 3)
    assert sum(s1 - s0 for s0, s1 in sp) / (sp[-1][1] - sp[0][0]) <= ROLL_MIN
    sums = []
    wants = [want_u8(f, tall[0], tall[1], None, size, sums=sums), want_u8(f, small[0], small[1], None, size)]
    assert clamps_at_both_ends(sums), sums
    outs, path = decode([tall[0], small[0]], None, size, name)
    assert path.endswith("+resize:" + name + "+roll"), path
    for i, o in enumerate(outs):
        assert np.array_equal(o, wants[i].reshape(-1)), (name, i, np.nonzero(o != wants[i].reshape(-1))[0][:10].tolist())
    outs, path = decode([small[0]], None, size, name)  # (no image takes the route: no mark)
    assert "+roll" not in path and np.array_equal(outs[0], wants[1].reshape(-1))
    for dtype in ("float32", "bfloat16"):
        fmt, ref_fmt = TN.fmt_of(dtype)
        outs, path = decode([tall[0], small[0], tall[0]], None, size, name, fmt, [True, False, False])
        assert path.endswith("+resize:" + name + "+tensor+roll"), path
        for i, o in enumerate(outs):
            want = T.bits(T.to_tensor(wants[i % 2], T.table(ref_fmt, 3), i == 0))
            assert np.array_equal(T.bits(o), want), (name, dtype, i)
    gray = block_case("gray", 64, 1080, 2, 1)
    outs, path = decode([gray[0]], None, size, name, rgb=True)  # (RGB output: the converting horizontal pass over the new rows)
    assert path.endswith("+rgb+resize:" + name + "+roll"), path
    assert np.array_equal(outs[0], want_u8(f, gray[0], gray[1], None, size, rgb=True).reshape(-1))


@pytest.mark.parametrize("name", WIDE)
def test_cmyk_on_the_run_route(name):
    """resample_run_body<4>: a CMYK 64 x 1080 source under RGB output to (224, 225) — the converting horizontal pass over the rows a run's
    bands do not share — as bytes and as f32 / f16 / bf16 tensors, flipped and not.  The conversion comes first: resampling the four
    inks and converting afterwards gives other bytes (asserted)."""
    f = F.NAMES[name]
    size = (224, 225)
    case, full = block_case("cmyk444", 64, 1080, 2, 1)
    rb, bands, cap, spans = plan_of(name, 1080, 224, 225, 3)
    assert bands >= 2 and all(s1 - s0 <= cap for s0, s1 in spans) and sum(s1 - s0 for s0, s1 in spans) / (spans[-1][1] - spans[0][0]) > ROLL_MIN, (rb, bands)
    sums = []
    want = want_u8(f, case, full, None, size, rgb=True, sums=sums)
    assert clamps_at_both_ends(sums), sums
    assert not np.array_equal(want, G.to_rgb(F.resize(RZ.source_of(case, full, None), 224, 225, f)))
    outs, path = decode([case], None, size, name, rgb=True)
    assert path.endswith("+rgb+resize:" + name + "+roll"), path
    assert np.array_equal(outs[0], want.reshape(-1)), np.nonzero(outs[0] != want.reshape(-1))[0][:10].tolist()
    for dtype in ("float32", "float16", "bfloat16"):
        fmt, ref_fmt = TN.fmt_of(dtype)
        outs, path = decode([case, case], None, size, name, fmt, [True, False], rgb=True)
        assert path.endswith("+rgb+resize:" + name + "+tensor+roll"), path
        for i, o in enumerate(outs):
            assert np.array_equal(T.bits(o), T.bits(T.to_tensor(want, T.table(ref_fmt, 3), i == 0))), (name, dtype, i)


@pytest.mark.parametrize("name", WIDE)
def test_forced_run_routes_give_the_band_route_s_bytes(monkeypatch, name):
    """JPGPU_RS_ROLL = 2 / 4 / 8 sends every candidate down the run route: the 97 x 61 image to (224, 225), which keeps its four bands by
    the rule (its rows overlap too little), decoded under each — plans the rule never picks, the bytes of knob `1`."""
    f = F.NAMES[name]
    size = (224, 225)
    cases = [block_case("420", 97, 61), block_case("gray", 97, 61), block_case("cmyk444", 97, 61)]  # (under RGB output: src_nc 0, 1 and 4)
    wins = None
    _rb, bands, cap, sp = plan_of(name, 61, 224, 225, 3)  # (a candidate that does not roll by the rule)
    assert bands >= 2 and all(s1 - s0 <= cap for s0, s1 in sp) and sum(s1 - s0 for s0, s1 in sp) / (sp[-1][1] - sp[0][0]) <= ROLL_MIN
    wants = [want_u8(f, case, full, None, size, rgb=True) for case, full in cases]
    fmt, ref_fmt = TN.fmt_of("float16")
    flips = [True, False, True]
    got = {}
    for knob in ("1", "2", "4", "8", None):
        if knob is None:
            monkeypatch.delenv("JPGPU_RS_ROLL", raising=False)
        else:
            monkeypatch.setenv("JPGPU_RS_ROLL", knob)
        outs, path = decode([c for c, _f in cases], wins, size, name, rgb=True)
        assert path.endswith("+roll") == (knob in ("2", "4", "8")), (knob, path)
        touts, tpath = decode([c for c, _f in cases], wins, size, name, fmt, flips, rgb=True)
        assert tpath.endswith("+tensor+roll" if knob in ("2", "4", "8") else "+tensor"), (knob, tpath)
        got[knob] = outs, touts
        for i, (o, t) in enumerate(zip(outs, touts)):
            assert np.array_equal(o, got["1"][0][i]) and np.array_equal(T.bits(t), T.bits(got["1"][1][i])), (name, knob, i)
            assert np.array_equal(o, wants[i].reshape(-1)), (name, knob, i, np.nonzero(o != wants[i].reshape(-1))[0][:10].tolist())
            assert np.array_equal(T.bits(t), T.bits(T.to_tensor(wants[i], T.table(ref_fmt, 3), flips[i]))), (name, knob, i)


def test_bilinear_by_name_is_the_call_without_a_filter():
    cases = [block_case("420", 97, 61), block_case("gray", 97, 61)]
    wins = [(5, 3, 87, 55), None]
    plain, path0 = RZ._decode([c for c, _f in cases], wins, (37, 53))
    for name in ("bilinear", 0, None):
        outs, path = decode([c for c, _f in cases], wins, (37, 53), name)
        assert path == path0 and ":" not in path, (path, path0)
        for o, w in zip(outs, plain):
            assert np.array_equal(o, w)
    bic, _p = decode([c for c, _f in cases], wins, (37, 53), "bicubic")
    assert not np.array_equal(bic[0], plain[0])  # (the filter bits are not ignored)


def test_batch_refusals():
    case, _full = block_case("420", 97, 61)
    N = J._native
    with pytest.raises(J.FormatError, match="filter 9"):
        J.Batch([RZ._desc(case)], output_size=(8, 8), filter=9)
    with pytest.raises(J.UnsupportedError, match="output size"):
        J.Batch([RZ._desc(case)], filter="lanczos")
    with pytest.raises(J.UnsupportedError, match="output size"):
        J.Batch([RZ._desc(case)], windows=[(1, 1, 9, 9)], flags=N.BATCH_FILTER(N.FILTER_BOX))


# ---- Pipeline: JPEG bytes in ---------------------------------------------------------------------------------------------------------
_FILES = {}


def block_file(layout, w, h, seed=0):
    """A baseline JPEG of 0 / 255 blocks of 8 x 8 pixels at quality 100 (tables of ones)."""
    key = (layout, w, h, seed)
    if key not in _FILES:
        rng = np.random.default_rng(100 + seed)
        a = rng.integers(0, 2, (-(-h // 8), -(-w // 8), 3), dtype=np.uint8) * np.uint8(255)
        if layout == "gray":
            a[:, :, 1] = a[:, :, 2] = a[:, :, 0]
        rgb = np.ascontiguousarray(a.repeat(8, axis=0).repeat(8, axis=1)[:h, :w])
        _FILES[key] = PW.BE.encode_rgb(rgb, 100, layout)
    return _FILES[key]


def _p_check(p, files, wins, out, size, name, fit=None, fmt=None, flips=None, rgb=False, label=""):
    f = F.NAMES[name]
    for i, data in enumerate(files):
        win = None if wins is None else wins[i]
        src, eff, (_W, _H, _nc) = RZ._p_source(data, None, None, win)
        src = G.to_rgb(src) if rgb else src
        assert not isinstance(out[i], Exception), (label, i, out[i])
        if fit is None:
            u8 = F.resize(src, size[0], size[1], f)
        else:
            pl = J.fit_placement(fit, (eff[2], eff[3]), size)
            assert p.placement(i) == pl
            u8 = F.placed(src, *pl, size[0], size[1], fit.fill, f)
        if fmt is None:
            assert np.array_equal(out[i], u8.reshape(-1)), (label, name, i, win)
        else:
            want = T.to_tensor(u8, T.table(fmt, u8.shape[2]), bool(flips[i]) if flips else False)
            assert np.array_equal(T.bits(out[i]), T.bits(want)), (label, name, i, win)


def test_pipeline_filter_changed_and_switched_off_between_calls():
    files = [block_file("420", 161, 97), block_file("444", 97, 61, 1), block_file("gray", 97, 61, 2), block_file("420", 161, 97, 3)]
    wins = [(5, 3, 151, 87), None, (1, 7, 95, 47), None]
    wins2 = [(7, 5, 121, 91), None, (3, 1, 81, 57), None]
    size = (37, 53)
    p = J.Pipeline(threads=4)
    try:
        plain = p.decode(files, windows=wins, output_size=size)
        path0 = p.kernel_path
        assert ":" not in path0 and "+resize" in path0
        _p_check(p, files, wins, plain, size, "bilinear", label="no filter")
        out = p.decode(files, windows=wins, output_size=size, filter="bicubic")
        assert ends(p.kernel_path, "+resize:bicubic"), p.kernel_path
        _p_check(p, files, wins, out, size, "bicubic", label="bicubic")
        assert not np.array_equal(out[0], plain[0])
        out = p.decode(files, windows=wins2, output_size=size, filter="bicubic")  # (fresh windows at the same filter: set in place)
        _p_check(p, files, wins2, out, size, "bicubic", label="bicubic, other windows")
        out = p.decode(files, windows=wins2, output_size=size, filter="lanczos")
        assert ends(p.kernel_path, "+resize:lanczos"), p.kernel_path
        _p_check(p, files, wins2, out, size, "lanczos", label="lanczos")
        for name in ("bilinear", None):  # (explicit bilinear: the bytes and the path string of no filter)
            out = p.decode(files, windows=wins, output_size=size, filter=name)
            assert p.kernel_path == path0
            for o, w in zip(out, plain):
                assert np.array_equal(o, w)
        full = p.decode(files, filter="bilinear")  # (no output size: what it always gave)
        PW._check_call(p, files, [None] * 4, full)
    finally:
        p.close()


def test_pipeline_refusals_leave_the_pipeline_usable():
    files = [block_file("420", 161, 97), block_file("gray", 97, 61, 2)]
    p = J.Pipeline(threads=2)
    try:
        with pytest.raises(J.FormatError, match="output size"):
            p.decode(files, filter="bicubic")  # (a filter without an output size: nothing is decoded)
        with pytest.raises(J.FormatError, match="filter 9"):
            p.decode(files, output_size=(37, 53), filter=9)
        out = p.decode(files, output_size=(37, 53), filter="hamming")
        _p_check(p, files, None, out, (37, 53), "hamming")
    finally:
        p.close()


def test_pipeline_clip_transform_and_letterbox():
    """CLIP's transform — the shorter side to the output's, bicubic, centre crop — as tensors with flips and RGB output; a letterbox
    with Lanczos."""
    files = [block_file("420", 161, 97), block_file("gray", 97, 61, 2), block_file("444", 97, 161, 4)]
    size = (48, 48)
    fmt, ref_fmt = TN.fmt_of("float32", T.CLIP)
    flips = [True, False, True]
    p = J.Pipeline(threads=2)
    try:
        fit = J.Fit("shorter_side_crop", size=48)
        out = p.decode(files, output_size=size, fit=fit, filter="bicubic", tensor=fmt, flips=flips, rgb=True)
        assert "+rgb+place+resize:bicubic+tensor" in p.kernel_path, p.kernel_path
        _p_check(p, files, None, out, size, "bicubic", fit, ref_fmt, flips, rgb=True, label="clip")
        fit = J.Fit("letterbox", fill=(114, 114, 114))
        out = p.decode(files, output_size=size, fit=fit, filter="lanczos")
        _p_check(p, files, None, out, size, "lanczos", fit, label="letterbox")
    finally:
        p.close()
