"""Windows of each image (jpgpu_batch_create_windowed, csrc/window_band.hpp) on the MI355X, bit-exact against the oracle's whole
decode sliced: every layout, scale and window shape of tests/test_window_emulation.py through the C ABI; mixed batches whose
unwindowed images keep their kernels and bytes; a caller's arena filled with a canary; windows the batch must refuse."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import synth
from test_window_emulation import LAYOUTS, grid_of, window_slice, windows_for

pytestmark = pytest.mark.gpu

J = None


@pytest.fixture(scope="module", autouse=True)
def _load():
    global J
    import jpeg_decoder_amd as pkg
    J = pkg
    assert J.device_count() >= 1, "no MI355X visible: the HIP path has no CPU fallback"


def to_j(comps):
    out = (J.Component * len(comps))()
    for i, c in enumerate(comps):
        out[i].identifier, out[i].horizontal_sampling_factor, out[i].vertical_sampling_factor = c.identifier, c.h, c.v
        out[i].quantization_table_index, out[i].dct_scale = c.tq, c.dct_scale
        out[i].size_width, out[i].size_height, out[i].block_width, out[i].block_height = c.size_w, c.size_h, c.block_w, c.block_h
    return out


def _case(rng, w_, h_, samp, ct, scale, kind):
    ocomps, _ = O.make_components(w_, h_, samp, dct_scale=scale)
    if kind == "sparse":
        qts = [rng.integers(1, 64, 64).astype(np.uint16) for _ in ocomps]
        coefs = [synth.sparse_coefficients(rng, c.block_w * c.block_h, amp=64, dc_amp=500) for c in ocomps]
    else:
        qts = [rng.integers(1, 65536, 64).astype(np.uint16) for _ in ocomps]
        coefs = [rng.integers(-32768, 32768, c.block_w * c.block_h * 64).astype(np.int16) for c in ocomps]
    ow, oh = J.scaled_output_size(w_, h_, scale)
    return ocomps, qts, coefs, ct, ow, oh


def _full(case):
    oc, qts, coefs, ct, ow, oh = case
    return O.pixels_from_coefficients(oc, qts, coefs, ow, oh, ct.upper())


def _desc(case):
    oc, qts, _c, ct, ow, oh = case
    return J.image_desc(list(to_j(oc)), qts, ow, oh, ct)


def _decode(cases, windows, flags=0, counts=None):
    b = J.Batch([_desc(c) for c in cases], flags=flags, windows=windows)
    try:
        for i, (oc, _q, coefs, *_r) in enumerate(cases):
            for c in range(len(oc)):
                b.upload(i, c, coefs[c])
        b.decode()
        b.synchronize()
        if counts is not None:
            counts.extend(b.class_counts())  # (images of the fused launch groups, per arithmetic class)
        return [b.download(i) for i in range(len(cases))], b.path
    finally:
        b.close()


def _want(case, full, win):
    oc, _q, _c, ct, ow, oh = case
    W, H = grid_of(oc, ow, oh)
    return full if win is None else window_slice(full, W, H, len(oc), ct, win)


SIZES = [(1, 1), (17, 9), (161, 97), (50, 34), (1920, 1080)]


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda l: f"{'_'.join(f'{h}{v}' for h, v in l[0])}-{l[1]}")
@pytest.mark.parametrize("scale", [8, 4, 2, 1])
@pytest.mark.parametrize("kind", ["sparse", "hostile"])
def test_batch_windows_bit_exact(layout, scale, kind):
    """One batch per layout and scale: every size, every window of windows_for() as an image of its own, in one launch."""
    samp, ct = layout
    rng = np.random.default_rng(scale * 1000 + len(samp) * 10 + (kind == "hostile"))
    cases, wins, fulls = [], [], []
    for (w_, h_) in SIZES:
        if w_ >= 1000 and kind == "hostile":
            continue
        case = _case(rng, w_, h_, samp, ct, scale, kind)
        try:
            full = _full(case)
        except O.OracleError:
            continue
        oc, *_r, ow, oh = case
        W, H = grid_of(oc, ow, oh)
        wl = windows_for(W, H, seed=W + H + scale)
        for win in (wl if w_ < 1000 else wl[::4]):  # (1080p: a quarter of them)
            cases.append(case)
            wins.append(win)
            fulls.append(full)
    if not cases:
        pytest.skip("the reference refuses every frame of this layout")
    outs, path = _decode(cases, wins)
    assert path in ("window", "mixed")
    for i, (case, win, full) in enumerate(zip(cases, wins, fulls)):
        want = _want(case, full, win)
        bad = np.nonzero(outs[i] != want)[0] if outs[i].size == want.size else np.arange(max(outs[i].size, want.size))
        assert bad.size == 0, (i, case[4], case[5], win, outs[i].size, want.size, bad[:10])


def test_whole_image_window_is_no_window():
    rng = np.random.default_rng(5)
    cases = [_case(rng, 161, 97, [(2, 2), (1, 1), (1, 1)], "YCbCr", 8, "sparse") for _ in range(3)]
    plain, path0 = _decode(cases, None)
    whole, path1 = _decode(cases, [(0, 0, 161, 97), None, (0, 0, 0, 0)])
    assert path0 == path1 == "fused420"
    for a, b_ in zip(plain, whole):
        assert np.array_equal(a, b_)


def test_mixed_batch_keeps_unwindowed_images_on_their_kernels():
    """Unwindowed images of a batch with windowed ones: their kernels (fused, scaled, generic) and their bytes stay as they are."""
    rng = np.random.default_rng(11)
    cases = [_case(rng, 640, 480, [(2, 2), (1, 1), (1, 1)], "YCbCr", 8, "sparse"),
             _case(rng, 640, 480, [(2, 2), (1, 1), (1, 1)], "YCbCr", 8, "hostile"),
             _case(rng, 333, 21, [(1, 1), (1, 1), (1, 1)], "RGB", 8, "sparse"),
             _case(rng, 250, 130, [(2, 2), (1, 1), (1, 1)], "YCbCr", 4, "sparse"),
             _case(rng, 64, 64, [(3, 1), (1, 1), (1, 1)], "YCbCr", 8, "sparse"),
             _case(rng, 640, 480, [(2, 2), (1, 1), (1, 1)], "YCbCr", 8, "sparse"),
             _case(rng, 300, 200, [(1, 1)], "Grayscale", 8, "sparse")]
    wins = [None, None, None, None, None, (100, 50, 333, 217), (7, 9, 100, 100)]
    n_plain, n_mixed = [], []
    plain, path_plain = _decode(cases[:5], None, counts=n_plain)
    outs, path = _decode(cases, wins, counts=n_mixed)
    assert path == "mixed" and path_plain == "mixed"
    # routing: the fused launch groups hold the same three images (two 4:2:0, one RGB) with the windowed ones added — a windowed
    # 4:2:0 image sent to the fused kernels would be counted there (its bytes alone would not tell: both kernels are exact)
    assert sum(n_plain) == 3 and n_mixed == n_plain, (n_plain, n_mixed)
    only_fused, p1 = _decode([cases[0], cases[5]], [None, (0, 0, 640, 480)], counts=[])
    assert p1 == "fused420"  # (a whole-image window is no window)
    _o, p2 = _decode([cases[0], cases[5]], [None, (1, 1, 638, 478)])
    assert p2 == "mixed"
    for i in range(5):
        assert np.array_equal(outs[i], plain[i]), i
    for i, (case, win) in enumerate(zip(cases, wins)):
        assert np.array_equal(outs[i], _want(case, _full(case), win)), i


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
    hip.hipFree.argtypes = [C.c_void_p]
    hip.hipMemset.argtypes = [C.c_void_p, C.c_int, C.c_size_t]
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


@pytest.mark.parametrize("scale", [8, 4, 2, 1])
def test_window_arena_canary(scale):
    """A caller's output arena filled with a canary: every byte of every window is written, no byte between images changes."""
    hip = _hip()
    rng = np.random.default_rng(300 + scale)
    layouts = [([(2, 2), (1, 1), (1, 1)], "YCbCr"), ([(1, 1)] * 3, "RGB"), ([(2, 1), (1, 1), (1, 1)], "YCbCr"), ([(1, 1)], "Grayscale"),
               ([(2, 2), (1, 1), (1, 1), (2, 2)], "YCCK"), ([(1, 1)] * 3, "None"), ([(4, 1), (1, 1), (1, 1)], "YCbCr")]
    sizes = [(250, 130), (1930, 40), (33, 17), (640, 480), (9, 300), (1025, 24), (64, 48)]
    cases = [_case(rng, w_, h_, samp, ct, scale, "sparse") for (samp, ct), (w_, h_) in zip(layouts, sizes)]
    wins = []
    for case in cases:
        oc, *_r, ow, oh = case
        W, H = grid_of(oc, ow, oh)
        w, h = max(1, W // 2 + 1), max(1, H // 3 + 1)
        wins.append((min(W - w, W // 5 + 1), min(H - h, H // 4), w, h) if W > 1 or H > 1 else None)
    b = J.Batch([_desc(c) for c in cases], flags=J._native.BATCH_EXTERNAL_BUFFERS, windows=wins)
    coef, out = C.c_void_p(), C.c_void_p()
    nco, nout = b.coef_arena_bytes(), b.out_arena_bytes()
    assert hip.hipMalloc(C.byref(coef), nco) == 0 and hip.hipMalloc(C.byref(out), nout + 4096) == 0
    try:
        b.bind(coef.value, out.value)
        for i, (oc, _q, coefs, *_r) in enumerate(cases):
            for c in range(len(oc)):
                b.upload(i, c, coefs[c])
        for pattern in (0xA5, 0x3C):
            assert hip.hipMemset(out, pattern, nout + 4096) == 0
            b.decode()
            b.synchronize()
            host = np.empty(nout + 4096, np.uint8)
            assert hip.hipMemcpy(host.ctypes.data, out, nout + 4096, 2) == 0
            covered = np.zeros(nout + 4096, bool)
            for i, (case, win) in enumerate(zip(cases, wins)):
                want = _want(case, _full(case), win)
                off = b.out_offset(i)
                assert b.out_bytes(i) == want.size
                got = host[off: off + want.size]
                bad = np.nonzero(got != want)[0]
                assert bad.size == 0, (scale, hex(pattern), i, win, bad[:16].tolist())
                covered[off: off + want.size] = True
            assert (host[~covered] == pattern).all(), "a kernel wrote outside the windows"
    finally:
        b.close()
        hip.hipFree(coef)
        hip.hipFree(out)


def test_window_outside_the_image_fails_creation():
    rng = np.random.default_rng(1)
    case = _case(rng, 64, 48, [(2, 2), (1, 1), (1, 1)], "YCbCr", 8, "sparse")
    for win in [(60, 0, 5, 1), (0, 48, 1, 1), (64, 0, 1, 1), (0, 40, 64, 9)]:
        with pytest.raises(J.FormatError, match="outside"):
            J.Batch([_desc(case)], windows=[win])
    # a hand-made descriptor the window planner cannot run (a block grid update_component_sizes does not make)
    oc, qts, *_r = case
    comps = list(to_j(oc))
    comps[1].block_width += 1
    J.Batch([J.image_desc(comps, qts, 64, 48, "YCbCr")]).close()  # (the whole-image kernels take it)
    with pytest.raises(J.UnsupportedError, match="block grid"):
        J.Batch([J.image_desc(comps, qts, 64, 48, "YCbCr")], windows=[(8, 8, 16, 16)])


def test_windows_at_every_scale_share_one_launch_grid():
    """Windowed images at dct_scales 8, 4, 2 and 1 in one batch: one launch per scale over one grid and one LDS size (the largest),
    every workgroup of the other scales' images leaving at once — each image still gets exactly its window."""
    rng = np.random.default_rng(4242)
    cases, wins = [], []
    for k, scale in enumerate([8, 4, 2, 1, 8, 4, 2, 1]):
        samp, ct = LAYOUTS[k % len(LAYOUTS)]
        w_, h_ = [(640, 480), (1930, 40), (250, 130), (161, 97)][k % 4]
        case = _case(rng, w_, h_, samp, ct, scale, "sparse")
        oc, *_r, ow, oh = case
        W, H = grid_of(oc, ow, oh)
        cases.append(case)
        wins.append((W // 7 | 1, H // 5, max(1, W // 2 | 1), max(1, H // 2)))
    outs, path = _decode(cases, wins)
    assert path == "window"
    for i, (case, win) in enumerate(zip(cases, wins)):
        assert np.array_equal(outs[i], _want(case, _full(case), win)), (i, case[4], case[5], win)


# ---- every launch group in one batch, on a caller's arenas, bound anew ------------------------------------------------------------------
_GROUPS = [  # (sampling, colour transform, scale, window): gray in front of colour, so the second image's first_plane_job is 1
    ([(1, 1)], "Grayscale", 8, None), ([(2, 2), (1, 1), (1, 1)], "YCbCr", 8, None),                    # fused (two plans)
    ([(1, 1)], "Grayscale", 2, None), ([(1, 1)] * 3, "YCbCr", 4, None),                                # scaled
    ([(1, 1)], "Grayscale", 4, (3, 5, 21, 13)), ([(2, 2), (1, 1), (1, 1)], "YCbCr", 8, (7, 3, 45, 31)),  # window
    ([(3, 1), (1, 1), (1, 1)], "YCbCr", 8, None), ([(3, 1), (1, 1), (1, 1)], "YCbCr", 8, None),        # generic: no fused kernel takes 3x1
    ([(1, 1)] * 3, "None", 8, None), ([(1, 1)] * 4, "None", 8, None)]                                # planar output (no output size)
_NEW_TABLES = (1, 2, 5, 6, 9)  # one image of each group gets other quantization tables in the second round


def _rebound_rounds(n_images, size):
    """Two rounds on one batch: decode on a first pair of caller-owned arenas; then other arenas, other pictures, other tables."""
    import resample_ref as R

    hip = _hip()
    rng = np.random.default_rng(83 * 59 + n_images)
    groups = _GROUPS[:n_images]
    first = [_case(rng, 83 + 2 * (i % 3), 59 + 2 * (i % 2), samp, ct, scale, "sparse") for i, (samp, ct, scale, _w) in enumerate(groups)]
    second = []
    for i, (oc, qts, _c, ct, ow, oh) in enumerate(first):
        _oc, new_q, coefs, *_r = _case(rng, 83 + 2 * (i % 3), 59 + 2 * (i % 2), groups[i][0], ct, groups[i][2], "sparse")
        second.append((oc, new_q if i in _NEW_TABLES else qts, coefs, ct, ow, oh))
    wins = [g[3] for g in groups]

    def want(case, win):
        if size is None:
            return _want(case, _full(case), win)
        oc, *_r, ow, oh = case
        W, H = grid_of(oc, ow, oh)
        x, y, w, h = win or (0, 0, W, H)
        src = window_slice(_full(case), W, H, len(oc), case[3], (x, y, w, h)).reshape(h, w, len(oc))
        return R.resize(src, size[0], size[1]).reshape(-1)

    b = J.Batch([_desc(c) for c in first], flags=J._native.BATCH_EXTERNAL_BUFFERS, windows=wins, output_size=size)
    nco, nout = b.coef_arena_bytes(), b.out_arena_bytes()
    arenas = [C.c_void_p() for _ in range(4)]
    try:
        assert b.path == ("mixed" if size is None else "mixed+resize")
        for a, nbytes in zip(arenas, (nco, nout, nco, nout)):
            assert hip.hipMalloc(C.byref(a), nbytes) == 0 and hip.hipMemset(a, 0x5A, nbytes) == 0
        outs = []
        for rnd, cases in enumerate((first, second)):
            b.bind(arenas[2 * rnd].value, arenas[2 * rnd + 1].value)
            for i, (oc, qts, coefs, *_r) in enumerate(cases):
                for c in range(len(oc)):
                    if rnd == 1 and i in _NEW_TABLES:
                        b.set_quantization_table(i, c, qts[c])
                    b.upload(i, c, coefs[c])
            b.decode()
            b.synchronize()
            outs.append([b.download(i) for i in range(n_images)])
            for i, case in enumerate(cases):
                w_ = want(case, wins[i])
                assert outs[rnd][i].size == w_.size and np.array_equal(outs[rnd][i], w_), (size, rnd, i, np.nonzero(outs[rnd][i] != w_)[0][:10].tolist())
        for i in range(n_images):
            assert not np.array_equal(outs[0][i], outs[1][i]), (size, i)
    finally:
        b.close()
        for a in arenas:
            hip.hipFree(a)


def test_every_launch_group_in_one_batch_rebound():
    """Two images of every launch group — the fused plans, the scaled, the window and the generic group — and two planar ones in ONE
    batch, each about 83 x 59 (several MCUs across and down, odd sizes), a gray image in front of a colour one inside each group:
    every image equals the oracle's decode (sliced where windowed); after other arenas are bound, other pictures uploaded and another
    quantization table set on one image of each group, every image equals the oracle again and differs from before.  The same with
    an output size for the eight images with interleaved output, against tests/resample_ref.py."""
    _rebound_rounds(10, None)
    _rebound_rounds(8, (40, 30))
