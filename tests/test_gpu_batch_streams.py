"""Batch calls on a caller's stream, with the host running ahead of the device: decode -> (ballast still running) -> new tables,
coefficients, arenas or flips -> decode, and one host synchronisation at the very end (include/jpgpu.h, "Batch calls on caller
streams").  A call that changes what a decode reads affects only decodes enqueued later: the decode still queued
behind the ballast must give the pixels of the state it was enqueued in.  tests/stream_harness.py makes the race deterministic
(ballast, the pending precondition, snapshots on the stream); every scenario runs on the null stream, a blocking stream and a
hipStreamNonBlocking one, for every launch group of the batch.

Safety: every scenario keeps one geometry, both arenas of a bind swap stay allocated, nothing grows an arena, and the first decode of a
batch (the one that allocates and binds) runs before the scenario starts — so an unordered rewrite can give wrong pixels, never an
access outside an allocation.

The precondition is asserted before every mutating call that follows a decode up to and including the first one that may wait for the
device itself: a dense jpgpu_batch_upload copies on the null stream behind the decode (that wait is the ordering under test), so only
the first of a row of uploads can find the decode pending.  Calls that touch host state only (tables, binds, flips) and compact uploads
from pinned memory never wait, and each of them finds it pending."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
import resample_ref as R
import rgb_ref as G
import tensor_ref as T
import test_gpu_call_sequences as CS
from stream_harness import KINDS, StreamHarness
from test_window_emulation import grid_of, window_slice

pytestmark = pytest.mark.gpu

J = None
NIMG = 3
L420, L444, LGRAY, L311, LCMYK = [(2, 2), (1, 1), (1, 1)], [(1, 1)] * 3, [(1, 1)], [(3, 1), (1, 1), (1, 1)], [(1, 1)] * 4
F16 = ("float16",) + T.CLIP

# name: (width, height, sampling, colour transform, dct_scale, window, output size, tensor, rgb, path)
GROUPS = {
    "fused420": (64, 48, L420, "YCbCr", 8, None, None, None, False, "fused420"),
    "fused444": (33, 17, L444, "YCbCr", 8, None, None, None, False, "fused444"),
    "fusedgray": (33, 17, LGRAY, "Grayscale", 8, None, None, None, False, "fusedgray"),
    "generic311": (70, 40, L311, "YCbCr", 8, None, None, None, False, "generic"),
    "scaled4": (64, 48, L420, "YCbCr", 4, None, None, None, False, "fused420-s4"),
    "scaled2": (64, 48, L420, "YCbCr", 2, None, None, None, False, "fused420-s2"),
    "scaled1": (64, 48, L420, "YCbCr", 1, None, None, None, False, "fused420-s1"),
    "window": (161, 97, L420, "YCbCr", 8, (33, 17, 31, 15), None, None, False, "window"),
    "resize": (50, 34, L420, "YCbCr", 8, None, (37, 53), None, False, "fused420+resize"),
    "resize-tensor-f16": (50, 34, L420, "YCbCr", 8, None, (37, 53), F16, False, "fused420+resize+tensor"),
    "rgb-resize-gray": (50, 34, LGRAY, "Grayscale", 8, None, (37, 53), None, True, "fusedgray+rgb+resize"),
    "rgb-resize-cmyk": (50, 34, LCMYK, "CMYK", 8, None, (37, 53), None, True, None),
}
GROUP_IDS = sorted(GROUPS)


@pytest.fixture(scope="module", autouse=True)
def _load():
    global J
    import jpeg_decoder_amd as pkg
    J = pkg
    CS.J = pkg
    assert J.device_count() >= 1, "no MI355X visible: the HIP path has no CPU fallback"


# ---- content and expected bytes, made once per group and never changed ----------------------------------------------------------------
_FIX, _WANT = {}, {}


def _fixture(name):
    """Per group: the components and, per letter, NIMG x (tables, coefficients) drawn as test_gpu_call_sequences._content draws them.
    'a', 'b', 'c': sparse pictures with tables of their own; 't': tables under which 'tight' is range class 3 and 'full' class 0."""
    if name not in _FIX:
        w, h, samp, _ct, scale = GROUPS[name][:5]
        rng = np.random.default_rng(4100 + GROUP_IDS.index(name))
        oc = O.make_components(w, h, samp, dct_scale=scale)[0]
        f = {"oc": oc, "out": J.scaled_output_size(w, h, scale), "q": {}, "c": {}}
        for letter in "abc":
            drawn = [CS._content(rng, oc, "sparse") for _ in range(NIMG)]
            f["q"][letter], f["c"][letter] = [d[0] for d in drawn], [d[1] for d in drawn]
        drawn = [CS._content(rng, oc, "tight") for _ in range(NIMG)]
        f["q"]["t"], f["c"]["tight"] = [d[0] for d in drawn], [d[1] for d in drawn]
        f["c"]["full"] = [CS._content(rng, oc, "full")[1] for _ in range(NIMG)]
        for i in range(NIMG):
            assert CS._exact_class(f["q"]["t"][i], f["c"]["tight"][i]) == 3 and CS._exact_class(f["q"]["t"][i], f["c"]["full"][i]) == 0
        _FIX[name] = f
    return _FIX[name]


def _want(name, i, q, c, flip=False):
    """The bytes image i of the group holds after a decode with tables `q` and coefficients `c` (letters of _fixture): the oracle's
    pixels, then the window, the RGB conversion, the resample and the tensor of the group, each by its numpy statement."""
    key = (name, i, q, c, bool(flip))
    if key not in _WANT:
        _w, _h, _samp, ct, _scale, win, size, tensor, rgb, _path = GROUPS[name]
        f = _fixture(name)
        oc, (ow, oh) = f["oc"], f["out"]
        full = O.pixels_from_coefficients(oc, f["q"][q][i], f["c"][c][i], ow, oh, ct.upper())
        W, H = grid_of(oc, ow, oh)
        nc = len(oc)
        if size is None:
            out = full if win is None else window_slice(full, W, H, nc, ct, win)
        else:
            x, y, ww, hh = win or (0, 0, W, H)
            src = window_slice(full, W, H, nc, ct, (x, y, ww, hh)).reshape(hh, ww, nc)
            u8 = R.resize(G.to_rgb(src) if rgb else src, size[0], size[1])
            out = u8 if tensor is None else T.bits(T.to_tensor(u8, T.table(tensor, u8.shape[2]), flip))
        _WANT[key] = np.ascontiguousarray(out).reshape(-1).view(np.uint8).copy()
    return _WANT[key]


def _batch(name, q, flags=0):
    w, h, _samp, ct, scale, win, size, tensor, rgb, path = GROUPS[name]
    f = _fixture(name)
    ow, oh = f["out"]
    descs = [J.image_desc(list(CS._to_j(f["oc"])), f["q"][q][i], ow, oh, ct) for i in range(NIMG)]
    fmt = None if tensor is None else J.TensorFormat(tensor[0], tensor[1], tensor[2])
    b = J.Batch(descs, flags=flags, windows=None if win is None else [win] * NIMG, output_size=size, tensor=fmt, rgb=rgb)
    if path is not None:
        assert b.path == path, (name, b.path)
    return b


def _upload(b, name, c, images=range(NIMG)):
    f = _fixture(name)
    for i in images:
        for k in range(len(f["oc"])):
            b.upload(i, k, f["c"][c][i][k])


def _set_tables(b, name, q, h, ev):
    """New tables on every component of every image; each call finds the decode in front of it pending."""
    f = _fixture(name)
    for i in range(NIMG):
        for k in range(len(f["oc"])):
            h.expect_pending(ev, f"set_quantization_table({i}, {k})")
            b.set_quantization_table(i, k, f["q"][q][i][k])


def _decode_snap(b, h, dst, arena=None):
    """ballast, decode, the event directly behind it, the snapshot of the output arena: all on the stream, no host wait."""
    h.ballast()
    b.decode(h.handle)
    ev = h.mark()
    h.snapshot(dst, b.out_arena() if arena is None else arena, b.out_arena_bytes())
    return ev


def _compare(b, name, snap, states, label):
    """snap: one host copy of a snapshot; states[i] = (q, c, flip) of image i at that decode."""
    bad = []
    for i, (q, c, flip) in enumerate(states):
        want = _want(name, i, q, c, flip)
        off = b.out_offset(i)
        assert b.out_bytes(i) == want.size, (name, i, b.out_bytes(i), want.size)
        got = snap[off: off + want.size]
        if not np.array_equal(got, want):
            others = [f"{qq}/{cc}" for qq in "abt" for cc in ("a", "b", "c", "tight", "full")
                      if (qq, cc) != (q, c) and (name, i, qq, cc, bool(flip)) in _WANT and np.array_equal(got, _WANT[(name, i, qq, cc, bool(flip))])]
            bad.append(f"image {i}: {int((got != want).sum())} of {want.size} bytes differ from tables {q!r} / coefficients {c!r}"
                       + (f" — they are those of {others[0]}" if others else ""))
    assert not bad, f"{label} ({b.path}): " + "; ".join(bad)


def _differ(name, s0, s1):
    """The precondition that makes a decode with the wrong state visible: the two states give other bytes for every image."""
    for i in range(NIMG):
        assert not np.array_equal(_want(name, i, *s0[i]), _want(name, i, *s1[i])), (name, i, s0[i], s1[i])


def _host(t):
    return t.cpu().numpy()


# ---- 1. other tables behind a decode -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", GROUP_IDS)
def test_tables_changed_behind_a_pending_decode(name, kind):
    """decode; set_quantization_table on every component; decode.  Snapshot 1 holds the pixels of the old tables (d_qt and, through
    the class that a new table resets, every job table go up before decode 2), snapshot 2 those of the new ones."""
    s1, s2 = [("a", "a", False)] * NIMG, [("b", "a", False)] * NIMG
    _differ(name, s1, s2)
    h = StreamHarness(kind)
    b = _batch(name, "a")
    try:
        _upload(b, name, "a")
        b.decode(h.handle)
        b.synchronize(h.handle)
        snaps = h.buffers(2, b.out_arena_bytes())
        ev = _decode_snap(b, h, snaps[0])
        _set_tables(b, name, "b", h, ev)
        _decode_snap(b, h, snaps[1])
        h.finish()
        got = _host(snaps)
        _compare(b, name, got[0], s1, "decode 1, old tables")
        _compare(b, name, got[1], s2, "decode 2, new tables")
    finally:
        h.close()
        b.close()


# ---- 2. other coefficients (and another arithmetic class) behind a decode ---------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("order", [("full", "tight"), ("tight", "full")], ids=["full-then-tight", "tight-then-full"])
@pytest.mark.parametrize("name", GROUP_IDS)
def test_dense_upload_behind_a_pending_decode(name, order, kind):
    """decode of class-0 coefficients; dense upload of class-3 ones; decode — and the reverse.  An upload that overtook the decode
    would give it the next picture's coefficients, and a class table that did would run it in the wrong arithmetic."""
    first, then = order
    s1, s2 = [("t", first, False)] * NIMG, [("t", then, False)] * NIMG
    _differ(name, s1, s2)
    h = StreamHarness(kind)
    b = _batch(name, "t")
    try:
        _upload(b, name, first)
        b.decode(h.handle)
        b.synchronize(h.handle)
        snaps = h.buffers(2, b.out_arena_bytes())
        ev = _decode_snap(b, h, snaps[0])
        h.expect_pending(ev, "the first dense upload")  # (the uploads behind it wait for the decode themselves)
        _upload(b, name, then)
        _decode_snap(b, h, snaps[1])
        h.finish()
        got = _host(snaps)
        _compare(b, name, got[0], s1, f"decode 1, {first} coefficients")
        _compare(b, name, got[1], s2, f"decode 2, {then} coefficients")
    finally:
        h.close()
        b.close()


# ---- 3. compact uploads: the expansion's job table ------------------------------------------------------------------------------------
def _compact(torch, name, q, c, i, k):
    """Component k of image i in the compact transport, in pinned memory (the copy is asynchronous: the buffer lives to the end)."""
    from jpeg_decoder_amd import _native as N
    f = _fixture(name)
    a = np.ascontiguousarray(f["c"][c][i][k], np.int16).reshape(-1)
    qq = np.ascontiguousarray(f["q"][q][i][k], np.uint16).reshape(64)
    buf = torch.empty(N.lib().jpgpu_compact_max_bytes(a.size // 64), dtype=torch.uint8).pin_memory()
    rc = C.c_int(0)
    n = N.lib().jpgpu_compact_encode(a.ctypes.data, a.size // 64, qq.ctypes.data, buf.data_ptr(), C.byref(rc))
    return buf, n, rc.value


def _send_compact(b, h, i, k, packed, classified):
    from jpeg_decoder_amd import _native as N
    buf, n, rc = packed
    b._check(N.lib().jpgpu_batch_upload_compact(b._h, i, k, buf.data_ptr(), n, rc if classified else -1, h.handle))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", GROUP_IDS)
def test_compact_upload_behind_a_pending_decode(name, kind):
    """upload_compact of every image; decode; upload_compact of other content for image 1 (classified) and image 2 (unclassified);
    decode.  The second expansion's job table is shorter and starts with another image: had it overtaken the first expansion, image 0
    would not have been expanded for decode 1."""
    s1 = [("a", "a", False)] * NIMG
    s2 = [("a", "a", False), ("a", "b", False), ("a", "b", False)]
    s0 = [("a", "c", False)] * NIMG
    _differ(name, s0, s1)
    h = StreamHarness(kind)
    b = _batch(name, "a")
    nk = len(_fixture(name)["oc"])
    try:
        packed = {(c, i, k): _compact(h.torch, name, "a", c, i, k) for c in "abc" for i in range(NIMG) for k in range(nk)}
        for i in range(NIMG):  # the first use of the transport and of the device-side classes allocates: before the scenario
            for k in range(nk):
                _send_compact(b, h, i, k, packed[("c", i, k)], classified=False)
        b.decode(h.handle)
        b.synchronize(h.handle)
        snaps = h.buffers(2, b.out_arena_bytes())
        for i in range(NIMG):
            for k in range(nk):
                _send_compact(b, h, i, k, packed[("a", i, k)], classified=True)
        ev = _decode_snap(b, h, snaps[0])
        for i in (1, 2):
            for k in range(nk):
                h.expect_pending(ev, f"upload_compact({i}, {k})")
                _send_compact(b, h, i, k, packed[("b", i, k)], classified=(i == 1))
        _decode_snap(b, h, snaps[1])
        h.finish()
        got = _host(snaps)
        _compare(b, name, got[0], s1, "decode 1, first compact uploads")
        _compare(b, name, got[1], s2, "decode 2, images 1 and 2 re-sent")
    finally:
        h.close()
        b.close()


# ---- 4. the caller's arenas: another output arena behind a decode -----------------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", GROUP_IDS)
def test_bind_behind_a_pending_decode(name, kind):
    """EXTERNAL_BUFFERS: decode into arena X; bind(coef, Y); new tables; decode.  X holds the first result (also after decode 2), Y the
    second, and Y's canary is intact in the snapshot taken between the two decodes."""
    s1, s2 = [("a", "a", False)] * NIMG, [("b", "a", False)] * NIMG
    _differ(name, s1, s2)
    h = StreamHarness(kind)
    torch = h.torch
    b = _batch(name, "a", flags=J._native.BATCH_EXTERNAL_BUFFERS)
    try:
        nout = b.out_arena_bytes()
        coef = torch.zeros(b.coef_arena_bytes(), dtype=torch.uint8, device="cuda")
        X = torch.full((nout,), 0x3C, dtype=torch.uint8, device="cuda")
        Y = torch.full((nout,), 0xA5, dtype=torch.uint8, device="cuda")
        assert coef.data_ptr() % 256 == 0 and X.data_ptr() % 256 == 0 and Y.data_ptr() % 256 == 0
        b.bind(coef.data_ptr(), X.data_ptr())
        _upload(b, name, "a")
        b.decode(h.handle)
        b.synchronize(h.handle)
        snaps = h.buffers(4, nout)
        torch.cuda.synchronize()
        ev = _decode_snap(b, h, snaps[0], X.data_ptr())
        h.expect_pending(ev, "bind")
        b.bind(coef.data_ptr(), Y.data_ptr())
        h.snapshot(snaps[1], Y.data_ptr(), nout)  # (between the two decodes, in stream order)
        _set_tables(b, name, "b", h, ev)
        _decode_snap(b, h, snaps[2], Y.data_ptr())
        h.snapshot(snaps[3], X.data_ptr(), nout)
        h.finish()
        got = _host(snaps)
        _compare(b, name, got[0], s1, "decode 1 into X")
        assert (got[1] == 0xA5).all(), f"{name}: {int((got[1] != 0xA5).sum())} bytes of Y were written before the decode that was given Y"
        _compare(b, name, got[2], s2, "decode 2 into Y")
        assert np.array_equal(got[3], got[0]), f"{name}: decode 2 changed X"
    finally:
        h.close()
        b.close()


# ---- 5. flips of a tensor batch (ordered on the stream already: a guard) --------------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
def test_flips_changed_behind_a_pending_decode(kind):
    name = "resize-tensor-f16"
    flips = [True, False, True]
    s1, s2 = [("a", "a", False)] * NIMG, [("a", "a", fl) for fl in flips]
    assert not np.array_equal(_want(name, 0, *s1[0]), _want(name, 0, *s2[0]))
    h = StreamHarness(kind)
    b = _batch(name, "a")
    try:
        _upload(b, name, "a")
        b.decode(h.handle)
        b.synchronize(h.handle)
        snaps = h.buffers(2, b.out_arena_bytes())
        ev = _decode_snap(b, h, snaps[0])
        h.expect_pending(ev, "set_flips")
        b.set_flips(flips)
        _decode_snap(b, h, snaps[1])
        h.finish()
        got = _host(snaps)
        _compare(b, name, got[0], s1, "decode 1, no flips")
        _compare(b, name, got[1], s2, "decode 2, images 0 and 2 flipped")
    finally:
        h.close()
        b.close()


# ---- 6. classes worked out on the stream, decode behind them with no host wait -----------------------------------------------------------
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("name", GROUP_IDS)
def test_classify_on_device_then_decode_without_a_host_wait(name, kind):
    """classify_on_device on the stream, decode on the stream: the pixels are those of the host's classification (the oracle's), and
    the class split promises no more than the exact classes — full, tight and sparse coefficients side by side."""
    contents = ["full", "tight", "full"]
    states = [("t", c, False) for c in contents]
    h = StreamHarness(kind)
    b = _batch(name, "t")
    f = _fixture(name)
    try:
        _upload(b, name, "tight")
        b.classify_on_device(h.handle)  # (the first use allocates the statistics and rebinds: before the scenario)
        b.decode(h.handle)
        b.synchronize(h.handle)
        for i, c in enumerate(contents):
            _upload(b, name, c, images=[i])
        snaps = h.buffers(1, b.out_arena_bytes())
        h.ballast()
        b.classify_on_device(h.handle)
        ev = _decode_snap(b, h, snaps[0])
        h.expect_pending(ev, "the end of the scenario")
        h.finish()
        _compare(b, name, _host(snaps)[0], states, "decode behind classify_on_device")
        exact = [CS._exact_class(f["q"]["t"][i], f["c"][c][i]) for i, c in enumerate(contents)]
        counts = b.class_counts()
        assert counts[2] <= sum(e == 3 for e in exact) and counts[1] + counts[2] <= sum(e >= 1 for e in exact), (name, counts, exact)
    finally:
        h.close()
        b.close()
