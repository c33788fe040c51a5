"""Windows from JPEG bytes: Pipeline.decode(windows=...) (jpgpu_pipeline_decode_windowed) on the MI355X.

Expected pixels everywhere: the oracle's whole decode of the same bytes (same scale request, same colour transform), reshaped and
sliced on the host, compared with np.array_equal.  Inputs: files under tests/golden/ and streams written by tools/baseline_encoder.py
and tools/progressive_encoder.py."""
import hashlib
import os
import sys

import numpy as np
import pytest

import oracle as O
import synth

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(_ROOT, "tools"))
import baseline_encoder as BE  # noqa: E402
import progressive_encoder as PE  # noqa: E402

pytestmark = pytest.mark.gpu
J = None
GOLDEN = os.path.join(_ROOT, "tests", "golden")
KNOBS = ("JPGPU_PIPE_ENTRY_PIXELS", "JPGPU_PIPE_PROG_DEVICE_PERCENT", "JPGPU_PROG_LANES_MAX", "JPGPU_PIPE_HOST_LIGHT", "JPGPU_PIPE_FORCE_DEVICE",
         "JPGPU_PIPE_FORCE_PEER_COPY", "JPGPU_PIPE_PROGRESSIVE_ON_HOST")


@pytest.fixture(scope="module", autouse=True)
def _load():
    global J
    import jpeg_decoder_amd as pkg
    J = pkg
    assert J.device_count() >= 1, "no MI355X visible: the HIP path has no CPU fallback"


# ---- files ---------------------------------------------------------------------------------------------------------------------------
_FILES, _WANT = {}, {}
SAMP4 = {"cmyk": [(2, 2), (1, 1), (1, 1), (1, 1)], "ycck-half": [(2, 2), (1, 1), (1, 1), (2, 2)]}


def _golden(*parts):
    with open(os.path.join(GOLDEN, *parts), "rb") as f:
        return f.read()


def _four_component_progressive(w, h, samp, seed):
    """A progressive frame of four components (no Adobe marker: the tests name the colour transform themselves)."""
    rng = np.random.default_rng(seed)
    comps, _ = J.make_components(w, h, samp)
    lum, chr_ = synth.quality_tables(85)
    qts = [lum, chr_, chr_, lum]
    coefs = [synth.sparse_coefficients(rng, int(c.block_width) * int(c.block_height), amp=64, dc_amp=500) for c in comps]
    script = [((0, 1, 2, 3), 0, 0, 0, 1), ((0, 1, 2, 3), 0, 0, 1, 0)] + [((c,), 1, 63, 0, 0) for c in range(4)]
    return PE.encode_from_coefficients(list(comps), qts, coefs, w, h, script)


def _file(layout, enc, size, pic=0):
    """layout: a sampling name of the encoders ("420", ..., "gray"), "cmyk", "ycck-half", "ycck"; enc: "base", "restart" (a marker per
    MCU row) or "prog".  Sequential four-component files come from tests/golden (their sizes are what they are)."""
    key = (layout, enc, size, pic)
    if key in _FILES:
        return _FILES[key]
    w, h = size
    if layout in BE.SAMPLINGS:
        rgb = synth.synthetic_rgb(w, h, seed=4000 + pic * 17 + w)
        if enc == "prog":
            data = PE.encode_rgb(rgb, PE.SPLIT_REFINEMENT_GRAY if layout == "gray" else PE.SPLIT_REFINEMENT_YCC, sampling=layout)
        else:
            hmax = max(hh for hh, _ in BE.SAMPLINGS[layout])
            data = BE.encode_rgb(rgb, 85, layout, restart_interval=(-(-w // (8 * hmax)) if enc == "restart" else 0))
    elif enc == "prog":
        data = _four_component_progressive(w, h, SAMP4[layout], seed=4000 + pic * 17 + w)
    elif layout == "cmyk":
        data = _golden("reftest", "mozilla", "jpg-cmyk-2.jpg" if w > 100 else "jpg-cmyk-1.jpg")
    else:  # "ycck": the golden YCCK file, and beside it a small CMYK one (another size in the same call)
        data = _golden("reftest", "ycck.jpg") if w > 100 else _golden("reftest", "mozilla", "jpg-cmyk-1.jpg")
    _FILES[key] = data
    return data


def _want(data, scale, ct):
    """(whole decode, W, H, nc) of the oracle for these bytes, scale request and colour transform; cached."""
    key = (hashlib.sha1(data).digest(), scale, ct)
    if key not in _WANT:
        d = O.decode(data, scale_to=scale, color_transform=(ct.upper() if ct else "AUTO"))
        W, H = (d.components[0].size_w, d.components[0].size_h) if d.ncomp == 1 else (d.width, d.height)
        assert d.pixels.size == W * H * d.ncomp
        _WANT[key] = (d.pixels, W, H, d.ncomp)
    return _WANT[key]


def _slice(full, W, H, nc, ct, win):
    if win is None:
        return full
    x, y, w, h = win
    if w == 0 or h == 0:
        return full
    if nc == 1:
        return full.reshape(H, W)[y:y + h, x:x + w].reshape(-1)
    if ct and ct.upper() == "NONE":
        return full.reshape(H, nc, W)[y:y + h, :, x:x + w].reshape(-1)
    return full.reshape(H, W, nc)[y:y + h, x:x + w].reshape(-1)


def windows_of(W, H):
    """On a 16-pixel grid, odd x / y / w / h, one pixel, one row, one column, touching each image edge, the whole image, None."""
    cand = [(16, 16, 32, 16), (13, 5, W - 20, H - 9), (5, 3, 7, 5), (1, 1, W - 2, H - 2), (W // 2, H // 2, 1, 1), (0, H // 3, W, 1),
            (W // 3 | 1, 0, 1, H), (0, 0, W // 2 + 1, H // 2 + 1), (W - 9, H - 7, 9, 7), (0, 0, W, H), None]
    out = []
    for win in cand:
        if win is None or (min(win) >= 0 and win[2] > 0 and win[3] > 0 and win[0] + win[2] <= W and win[1] + win[3] <= H):
            if win not in out:
                out.append(win)
    return out


def _env(monkeypatch, env):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)


def _check_call(p, files, wins, out, scale=None, ct=None, label=""):
    """Every image of the call against the oracle's slice; window(i), info(i) and the byte counts as specified."""
    bad = []
    for i, (data, win) in enumerate(zip(files, wins)):
        full, W, H, nc = _want(data, scale, ct)
        want = _slice(full, W, H, nc, ct, win)
        got = out[i]
        if isinstance(got, Exception):
            bad.append((i, win, repr(got)))
            continue
        if not np.array_equal(got, want):
            bad.append((i, win, (W, H, nc), got.size, want.size))
        eff = (0, 0, W, H) if (win is None or win[2] == 0 or win[3] == 0) else tuple(win)
        assert p.window(i) == eff, (label, i, p.window(i), eff)
        assert J._native.lib().jpgpu_pipeline_pixel_bytes(p._h, i) == eff[2] * eff[3] * nc, (label, i)
        inf = p.info(i)
        if nc > 1:
            assert (inf.width, inf.height) == (W, H), (label, i, inf)
    assert not bad, (label, bad[:8], len(bad))


# ---- 1. the matrix ---------------------------------------------------------------------------------------------------------------------
ROUTES = {
    "host-compact": ("base", {"device_entropy": False}, {}),
    "host-dense": ("base", {"device_entropy": False, "dense": True}, {}),
    "device": ("base", {}, {"JPGPU_PIPE_FORCE_DEVICE": "1"}),
    "device-restart": ("restart", {}, {"JPGPU_PIPE_FORCE_DEVICE": "1"}),
    "host-staged": ("base", {"host_light": False}, {"JPGPU_PIPE_FORCE_DEVICE": "1"}),
    "prog-device": ("prog", {}, {"JPGPU_PIPE_PROG_DEVICE_PERCENT": "100"}),
    "prog-host": ("prog", {"progressive_on_host": True}, {}),
}
# layout -> (file layout, colour transform to set, sizes)
LAYOUTS = {
    "420": ("420", None, [(161, 97), (50, 34)]), "422": ("422", None, [(161, 97), (50, 34)]), "444": ("444", None, [(161, 97), (50, 34)]),
    "gray": ("gray", None, [(161, 97), (50, 34)]), "440": ("440", None, [(161, 97), (50, 34)]), "411": ("411", None, [(161, 97), (50, 34)]),
    "cmyk": ("cmyk", "CMYK", [(256, 256), (32, 32)]), "ycck-half": ("ycck-half", "YCCK", [(161, 97), (50, 34)]),
    "ycck": ("ycck", None, [(500, 333), (32, 32)]), "none": ("444", "None", [(161, 97), (50, 34)]),
}
SCALES = [8, 4, 2, 1]


def _feasible(route, layout):
    enc = ROUTES[route][0]
    if layout == "ycck-half":
        return enc == "prog"  # (the baseline encoder writes one or three components; the golden YCCK file has full-size components)
    if layout in ("cmyk", "ycck"):
        return enc == "base"  # golden files: sequential, no restart markers; the four-component progressive frames are "ycck-half"
    return True


MATRIX = [(r, l, SCALES[(ri + li) % 4]) for ri, r in enumerate(ROUTES) for li, l in enumerate(LAYOUTS) if _feasible(r, l)]


def test_matrix_covers_every_route_layout_and_scale():
    assert {m[0] for m in MATRIX} == set(ROUTES) and {m[1] for m in MATRIX} == set(LAYOUTS)
    for r in ROUTES:
        assert len({m[2] for m in MATRIX if m[0] == r}) >= 3, r
    assert {m[2] for m in MATRIX} == set(SCALES)
    for l in LAYOUTS:
        assert len({m[2] for m in MATRIX if m[1] == l}) >= 2, l


@pytest.mark.parametrize("route,layout,s", MATRIX, ids=[f"{r}-{l}-s{s}" for r, l, s in MATRIX])
def test_windows_matrix(monkeypatch, route, layout, s):
    """One call per case: two image sizes, every window shape of windows_of() as an image of its own, windowed and unwindowed mixed."""
    enc, kwargs, env = ROUTES[route]
    flayout, ct, sizes = LAYOUTS[layout]
    big = sizes[0]
    scale = None if s == 8 else (-(-big[0] * s // 8), -(-big[1] * s // 8))
    files, wins = [], []
    for k, size in enumerate(sizes):
        data = _file(flayout, enc, size, pic=k)
        _full, W, H, _nc = _want(data, scale, ct)
        for win in windows_of(W, H):
            files.append(data)
            wins.append(win)
    odd = [w for w in wins if w is not None and (w[0] % 2 and w[1] % 2 and w[2] % 2 and w[3] % 2)]
    assert odd, "fixture: no odd window in this call"
    _env(monkeypatch, env)
    p = J.Pipeline(threads=4)
    try:
        out = p.decode(files, scale=scale, color_transform=ct, windows=wins, **kwargs)
        t = p.timings()
        _check_call(p, files, wins, out, scale, ct, label=f"{route} {layout} s{s}")
        n_win = sum(1 for f, w in zip(files, wins) if w is not None and w != (0, 0) + _want(f, scale, ct)[1:3])
        assert t["images_windowed"] == n_win and t["images_ok"] == len(files), t
        if layout in BE.SAMPLINGS or layout == "none":  # (files of the encoders: the routes are known)
            if route in ("device", "device-restart", "host-staged"):
                assert t["images_device_entropy"] == len(files) and t["images_device_rejected"] == 0 and t["images_device_progressive"] == 0, t
                assert (t["images_host_light"] == 0) == (route != "device"), t
            elif route == "prog-device":
                assert t["images_device_progressive"] == len(files) and t["images_device_rejected"] == 0, t
            else:
                assert t["images_device_entropy"] == 0, t
    finally:
        p.close()


def test_windows_with_pinned_input(monkeypatch):
    _env(monkeypatch, {"JPGPU_PIPE_FORCE_DEVICE": "1"})
    files, wins = [], []
    for k, size in enumerate([(161, 97), (333, 200)]):
        data = _file("420", "base", size, pic=k)
        for win in windows_of(*size):
            files.append(data)
            wins.append(win)
    arena = J.PinnedFiles(files)
    p = J.Pipeline(threads=4)
    try:
        out = p.decode(arena, input_pinned=True, windows=wins)
        t = p.timings()
        assert t["input_pinned"] == 1 and t["images_device_entropy"] == len(files), t
        _check_call(p, files, wins, out, label="pinned input")
    finally:
        p.close()
        arena.close()


# ---- 2. routing --------------------------------------------------------------------------------------------------------------------------
def test_windowed_420_images_leave_the_entry_list_walk_to_the_others(monkeypatch):
    _env(monkeypatch, {})
    n = 64
    files = [_file("420", "base", (333, 200), pic=k % 8) for k in range(n)]
    wins = [(13 + k, 5, 101, 77) if k % 2 else None for k in range(n)]
    p = J.Pipeline(threads=4)
    try:
        out = p.decode(files, windows=wins)
        t = p.timings()
        assert t["images_device_entropy"] == n and t["images_device_rejected"] == 0, t
        assert t["images_entry_pixels"] == n // 2 and t["images_windowed"] == n // 2, t
        _check_call(p, files, wins, out, label="half windowed")
        # whole-image windows (and empty ones) change no counter and no kernel path against windows=None
        out0 = p.decode(files)
        t0, path0 = p.timings(), p.kernel_path
        whole = [(0, 0, 333, 200) if k % 3 else ((0, 0, 0, 0) if k % 2 else None) for k in range(n)]
        out1 = p.decode(files, windows=whole)
        t1, path1 = p.timings(), p.kernel_path
        assert path0 == path1 == "fused420", (path0, path1)
        for k in ("images_ok", "images_device_entropy", "images_device_rejected", "images_entry_pixels", "images_windowed", "images_host_light",
                  "images_device_progressive", "pixel_bytes", "coefficient_bytes"):
            assert t0[k] == t1[k], (k, t0[k], t1[k])
        assert t1["images_windowed"] == 0 and t1["images_entry_pixels"] == n
        for a, b in zip(out0, out1):
            assert np.array_equal(a, b)
    finally:
        p.close()


# ---- 3. sizes and the three ways to the pixels ------------------------------------------------------------------------------------------
def test_window_bytes_by_every_download_mode(monkeypatch):
    _env(monkeypatch, {})
    files = [_file("420", "base", (333, 200), pic=k) for k in range(6)] + [_file("gray", "base", (161, 97), pic=1)]
    wins = [(13, 5, 101, 77), None, (0, 0, 333, 200), (332, 199, 1, 1), (0, 7, 333, 1), (16, 16, 64, 32), (5, 3, 7, 5)]
    p = J.Pipeline(threads=4)
    try:
        a = p.decode(files, windows=wins, download=True)
        _check_call(p, files, wins, a, label="download=True")
        t = p.timings()
        assert t["pixel_bytes"] == sum(x.size for x in a), t
        counts = p.decode(files, windows=wins, download="pinned")
        assert counts == [x.size for x in a]
        b = [p.pixels_host(i).copy() for i in range(len(files))]
        counts = p.decode(files, windows=wins, download=False)
        assert counts == [x.size for x in a]
        assert p.pixels_host(0) is None
        c = [p.download(i) for i in range(len(files))]
        for i in range(len(files)):
            assert np.array_equal(a[i], b[i]) and np.array_equal(a[i], c[i]), i
            assert p.device_pointer(i)
    finally:
        p.close()


# ---- 4. errors are per image ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("device_entropy", [True, False], ids=["device", "host"])
def test_errors_are_per_image(monkeypatch, device_entropy):
    _env(monkeypatch, {"JPGPU_PIPE_FORCE_DEVICE": "1"})
    good = _file("420", "base", (333, 200), pic=0)
    damaged = bytearray(_file("420", "base", (333, 200), pic=1))
    cut = len(damaged) * 2 // 3
    damaged = bytes(damaged[:cut])  # the scan ends early (no EOI): whatever the decoder makes of it, with and without a window
    unreadable = b"\xff\xd8\xff\xe0\x00\x03"
    scale = (167, 100)  # -> 1/2: 167 x 100
    files = [good, good, unreadable, damaged, good, good]
    wins = [(300, 100, 40, 40), (100, 50, 80, 60), None, (13, 5, 101, 77), (13, 5, 101, 77), None]
    p = J.Pipeline(threads=4)
    try:
        plain = p.decode(files[:], device_entropy=device_entropy)  # the unwindowed call: what the damaged file gives on its own
        out = p.decode(files, windows=wins, device_entropy=device_entropy)
        assert isinstance(out[0], J.FormatError) and "window" in str(out[0]) and "333x200" in str(out[0]), out[0]
        assert not isinstance(out[1], Exception)
        assert isinstance(out[2], Exception) and type(out[2]) is type(plain[2]) and str(out[2]) == str(plain[2])
        if isinstance(plain[3], Exception):
            assert type(out[3]) is type(plain[3]) and str(out[3]) == str(plain[3])
        else:
            assert np.array_equal(out[3], _slice(plain[3], 333, 200, 3, None, wins[3]))
        for k in (1, 4, 5):
            full, W, H, nc = _want(files[k], None, None)
            assert np.array_equal(out[k], _slice(full, W, H, nc, None, wins[k])), k
        assert p.window(0) is None and p.info(0).width == 333 and p.window(2) is None
        # a window outside only once the image is scaled
        out = p.decode(files, windows=wins, scale=scale, device_entropy=device_entropy)
        assert isinstance(out[0], J.FormatError)
        assert isinstance(out[1], J.FormatError) and "167x100" in str(out[1]), out[1]
        assert isinstance(out[2], Exception)
        for k in (4, 5):
            full, W, H, nc = _want(files[k], scale, None)
            assert (W, H) == (167, 100)
            assert np.array_equal(out[k], _slice(full, W, H, nc, None, wins[k])), k
        assert p.info(1).width == 167
    finally:
        p.close()


# ---- 5. reuse ---------------------------------------------------------------------------------------------------------------------------
N = 64
GEOM = (333, 200)


def _windows_set(name, n):
    W, H = GEOM
    if name == "A":
        return [(13 + k % 50, 5 + k % 30, 101, 77) for k in range(n)]
    if name == "B":  # the sizes of A at other positions: the byte counts, offsets and buffers are A's
        return [(150 - k % 50, 100 - k % 30, 101, 77) for k in range(n)]
    if name == "C":
        return [(7 + k % 20, 3 + k % 10, 33 + 2 * (k % 40), 21 + k % 50) for k in range(n)]
    if name == "whole":
        return [(0, 0, W, H)] * n
    if name == "half":  # every other image
        return [(13 + k % 50, 5 + k % 30, 101, 77) if k % 2 else None for k in range(n)]
    return None


CALLS = {
    "device": ("base", {}, {}),
    "prog": ("prog", {}, {"JPGPU_PIPE_PROG_DEVICE_PERCENT": "100"}),
    "host": ("base", {"device_entropy": False}, {}),
}


def _reuse_sequence(monkeypatch, p, steps, n):
    """steps: (call kind, window set).  Slot k of call c holds picture (k + n/2 * (c % 2)) mod n: no slot sees the same picture in two
    consecutive calls, so a call that left the previous call's pixels in place cannot pass."""
    bad = []
    for c, (kind, wname) in enumerate(steps):
        enc, kwargs, env = CALLS[kind]
        _env(monkeypatch, env)
        files = [_file("420", enc, GEOM, pic=(k + n // 2 * (c % 2)) % n) for k in range(n)]
        wins = _windows_set(wname, n)
        out = p.decode(files, windows=wins, **kwargs)
        t = p.timings()
        assert t["images_ok"] == n and t["images_device_rejected"] == 0, (c, kind, wname, t)
        for k in range(n):
            full, W, H, nc = _want(files[k], None, None)
            want = _slice(full, W, H, nc, None, wins[k] if wins else None)
            if isinstance(out[k], Exception) or not np.array_equal(out[k], want):
                bad.append((c, kind, wname, k))
    assert not bad, (bad[:10], len(bad))


def test_reuse_with_changing_windows(monkeypatch):
    p = J.Pipeline(threads=4)
    try:
        _reuse_sequence(monkeypatch, p, [("device", w) for w in ("A", "B", "C", None, "A", "whole", "half", "A", "A", "B", "half", "C")], N)
    finally:
        p.close()


def test_reuse_with_changing_windows_and_call_kinds(monkeypatch):
    p = J.Pipeline(threads=4)
    try:
        steps = [("device", "A"), ("prog", "B"), ("host", "A"), ("device", "B"), ("host", "C"), ("prog", None), ("device", "A"),
                 ("prog", "A"), ("prog", "B"), ("host", "B"), ("host", "whole"), ("device", "half"), ("prog", "half"), ("device", None),
                 ("device", "C"), ("host", None), ("host", "A")]
        _reuse_sequence(monkeypatch, p, steps, N)
    finally:
        p.close()


# ---- 6. the multi-device object on one GPU ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gather,force_peer", [(False, False), (True, False), (True, True)], ids=["plain", "gather", "gather-peer-copy"])
def test_two_children_on_one_device(monkeypatch, gather, force_peer):
    _env(monkeypatch, {"JPGPU_PIPE_FORCE_PEER_COPY": "1"} if force_peer else {})
    n = 96
    files = [_file("420", "base", (333, 200) if k % 3 else (161, 97), pic=k % 8) for k in range(n)]
    wins = [None if k % 5 == 0 else ((13 + k, 5 + k % 9, 41 + 2 * (k % 20), 33) if k % 3 else (5, 3, 7 + 2 * (k % 30), 5 + k % 40)) for k in range(n)]
    p = J.Pipeline(devices=[0, 0], threads=4)
    try:
        out = p.decode(files, windows=wins, gather=gather, download=False)
        t = p.timings()
        assert t["images_ok"] == n and t["images_windowed"] == sum(w is not None for w in wins), t
        if gather:
            assert t["gather_bytes"] > 0
        assert all(p.device_of(i) == (0, 0) for i in range(n))
        got = [p.download(i) for i in range(n)]
        _check_call(p, files, wins, got, label="two children")
        if gather:  # the gathered copy holds the windows' bytes at the pointers the object hands out
            import ctypes as C
            hip = C.CDLL("libamdhip64.so")
            hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
            for i in range(n):
                buf = np.empty(got[i].size, np.uint8)
                assert hip.hipMemcpy(buf.ctypes.data, p.device_pointer(i), buf.size, 2) == 0
                assert np.array_equal(buf, got[i]), i
        out = p.decode(files, windows=wins, gather=gather)
        _check_call(p, files, wins, out, label="two children, downloaded")
    finally:
        p.close()


# ---- 7. a loader's call ---------------------------------------------------------------------------------------------------------------------
def random_resized_crops(rng, n, W, H):
    """RandomResizedCrop: 8-100 % of the area, aspect 3/4-4/3 (log-uniform), any coordinates."""
    out = []
    while len(out) < n:
        area = W * H * rng.uniform(0.08, 1.0)
        ar = np.exp(rng.uniform(np.log(3 / 4), np.log(4 / 3)))
        w, h = int(round(np.sqrt(area * ar))), int(round(np.sqrt(area / ar)))
        if 0 < w <= W and 0 < h <= H:
            out.append((int(rng.integers(0, W - w + 1)), int(rng.integers(0, H - h + 1)), w, h))
    return out


def test_1024_files_of_1080p_with_random_resized_crops(monkeypatch):
    _env(monkeypatch, {})
    n, distinct = 1024, 8
    pics = [BE.synthetic_jpeg(1920, 1080, seed=9000 + k) for k in range(distinct)]
    fulls = [O.decode(d).pixels.reshape(1080, 1920, 3) for d in pics]
    rng = np.random.default_rng(20261016)
    wins = random_resized_crops(rng, n, 1920, 1080)
    assert any(w[0] % 2 and w[1] % 2 for w in wins)
    files = [pics[k % distinct] for k in range(n)]
    p = J.Pipeline()
    try:
        counts = p.decode(files, windows=wins, download="pinned")
        t = p.timings()
        assert t["images_ok"] == n and t["images_device_rejected"] == 0 and t["images_windowed"] == sum(w != (0, 0, 1920, 1080) for w in wins), t
        assert t["images_entry_pixels"] == n - t["images_windowed"]
        bad = []
        for i, (x, y, w, h) in enumerate(wins):
            want = hashlib.sha256(np.ascontiguousarray(fulls[i % distinct][y:y + h, x:x + w])).digest()
            got = p.pixels_host(i)
            if counts[i] != w * h * 3 or hashlib.sha256(got).digest() != want:
                bad.append((i, wins[i]))
        assert not bad, (bad[:10], len(bad))
    finally:
        p.close()


# ---- 8. the expansion limited to the rows a window reads (JPGPU_PIPE_WINDOW_ROWS) ----------------------------------------------------------
def _uniform_table_file(w, h, sampling, seed, restart_interval=0):
    """Every component with the same quantization table: the encoder then gives them the same Huffman tables too — a `uniform` scan,
    whose DC values the device sums over the whole plane after the expansion (huff_dc_prefix_kernel)."""
    rgb = synth.synthetic_rgb(w, h, seed=seed)
    comps, _ = J.make_components(w, h, BE.SAMPLINGS[sampling])
    lum, _chr = synth.quality_tables(85)
    qts = [lum, lum, lum]
    coefs = synth.coefficients_from_rgb(rgb, comps, "ycbcr", qts)
    return BE.encode_from_coefficients(list(comps), qts, coefs, w, h, restart_interval)


@pytest.mark.parametrize("host_light", [None, False], ids=["light", "staged"])
def test_row_limited_expansion_changes_no_byte(monkeypatch, host_light):
    files, wins = [], []

    def add(data, W, H, mcu):
        for win in [(0, 0, W, 5), (0, 0, 7, 3), (0, H - 3, W, 3), (W - 5, H - 1, 5, 1), (13, mcu + 1, W - 20, mcu - 2), (5, 3, 7, 5), (W // 2, H // 2, 1, 1),
                    (1, 2 * mcu - 1, W - 2, 2), (0, mcu, W, mcu), None]:
            files.append(data)
            wins.append(win)

    add(_file("420", "base", (333, 200)), 333, 200, 16)
    add(_file("420", "restart", (333, 200), pic=1), 333, 200, 16)
    add(_file("422", "base", (161, 97)), 161, 97, 8)
    add(_file("440", "restart", (161, 97)), 161, 97, 16)
    add(_file("411", "base", (161, 97)), 161, 97, 8)
    add(_uniform_table_file(250, 130, "444", 31), 250, 130, 8)
    add(_uniform_table_file(250, 130, "420", 32), 250, 130, 16)
    add(_uniform_table_file(250, 130, "420", 33, restart_interval=16), 250, 130, 16)
    add(_golden("reftest", "rgb.jpg"), 500, 333, 8)
    add(_golden("reftest", "mozilla", "jpg-cmyk-2.jpg"), 256, 256, 16)
    p = J.Pipeline(threads=4)
    try:
        outs = {}
        for knob in ("1", "0", "1"):
            _env(monkeypatch, {"JPGPU_PIPE_FORCE_DEVICE": "1"})
            monkeypatch.setenv("JPGPU_PIPE_WINDOW_ROWS", knob)
            out = p.decode(files, windows=wins, host_light=host_light)
            t = p.timings()
            assert t["images_device_entropy"] >= 90 and t["images_device_rejected"] == 0, t
            _check_call(p, files, wins, out, label=f"JPGPU_PIPE_WINDOW_ROWS={knob}")
            outs.setdefault(knob, out)
        for a, b in zip(outs["1"], outs["0"]):
            assert np.array_equal(a, b)
    finally:
        monkeypatch.delenv("JPGPU_PIPE_WINDOW_ROWS", raising=False)
        p.close()
