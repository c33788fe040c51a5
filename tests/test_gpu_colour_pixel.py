"""HUE and SHARPNESS (csrc/colour_pixel_band.hpp) on the MI355X: through jpgpu_colour_apply on a caller's pixels — the
device arithmetic of HUE over all 2^24 colours, SHARPNESS at every strip height — through Batch behind the fixed output size, and
through Pipeline.decode from JPEG bytes.  The expected value is always tests/colour_pixel_ref.py (the numpy statement, pinned to Pillow
by tests/golden/colour_pixel), on the references the other colour tests use, compared with np.array_equal."""
import numpy as np
import pytest

import colour_pixel_ref as PR
import tensor_ref as T
import test_gpu_colour as GC
import test_gpu_pipeline_colour as GP
import test_gpu_pipeline_windows as PW
import test_gpu_resize as RZ
import test_gpu_tensor as TN
import warp_ref as WR
from stream_harness import StreamHarness

pytestmark = pytest.mark.gpu

J = None
torch = None
JITTER = [("hue", 43), ("brightness", 1.2), ("contrast", 0.8), ("saturation", 1.3)]
PROGRAMS = [[("hue", 43)], [("hue", 0)], [("sharpen", 1.9)], [("sharpen", 0.37)], JITTER, [JITTER[2], JITTER[3], JITTER[0], JITTER[1]], [("sharpen", 1.9), ("equalize", 0)],
            [("sharpen", 256.0)], [("hue", 213), ("sharpen", 0.0)], None]
FACTORS = (0.0, 0.37, 1.9, 256.0)


@pytest.fixture(scope="module", autouse=True)
def _load():
    global J, torch
    import torch as th

    import jpeg_decoder_amd as pkg
    J, torch = pkg, th
    for m in (GC, GP, PW, RZ, TN):
        m.J = pkg
    assert J.device_count() >= 1, "no MI355X visible: the HIP path has no CPU fallback"


@pytest.fixture(scope="module")
def round_trip():
    return PR.RoundTrip()


def rows_env(monkeypatch, rows):
    if rows:
        monkeypatch.setenv("JPGPU_CL_STRIP_ROWS", str(rows))
    else:
        monkeypatch.delenv("JPGPU_CL_STRIP_ROWS", raising=False)


def want_u8(r, program, flip=False, warp=None, m=None):
    c = PR.apply(r, program)
    c = c[:, ::-1] if flip else c
    if warp is None:
        return np.ascontiguousarray(c)
    return WR.warp(c, WR.IDENTITY if m is None else m, WR.BILINEAR if warp == "bilinear" else WR.NEAREST, GC.WFILL)


# ---- programs on a caller's pixels ----

@pytest.mark.parametrize("shift", [1, 43, 213])
def test_colour_apply_hue_over_every_colour(round_trip, shift):
    t = torch.from_numpy(PR.all_colours()).cuda()
    assert J.colour_apply(t, [[("hue", shift)]] * 4) is t
    got, want = t.cpu().numpy(), round_trip.hue(shift)
    assert np.array_equal(got, want), np.argwhere((got != want).any(-1))[:8].tolist()


def images(W, H, seed):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, 256, (H, W, 3), dtype=np.uint8), PR.make_input({"const": [9, 200, 77], "H": H, "W": W}), PR.make_input({"checker": 1, "H": H, "W": W}),
                     rng.integers(90, 130, (H, W, 3), dtype=np.uint8)])


@pytest.mark.parametrize("size", [(4, 3), (5, 4), (36, 17), (224, 224), (2048, 8)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_colour_apply_sharpness_at_every_strip_height(monkeypatch, size):
    """Random, constant and checkerboard images, four a call (3 W H is a multiple of 4 at these sizes: the base rule of jpgpu_colour_apply
    refuses 3 x 3 and 33 x 17, which test_batch_u8_bit_exact runs instead), at the default strip height and at 1, 2 and 3 rows."""
    W, H = size
    P = images(W, H, 2200 + W)
    want = {f: np.stack([PR.apply(p, [("sharpen", f)]) for p in P]) for f in FACTORS}
    assert not np.array_equal(want[1.9][0], P[0]) and not np.array_equal(want[0.0][2], P[2])  # (the operation does something)
    for rows in (0, 1, 2, 3):
        rows_env(monkeypatch, rows)
        for f in FACTORS:
            t = torch.from_numpy(P).cuda()
            J.colour_apply(t, [[J.sharpness(f)]] * 4)
            got = t.cpu().numpy()
            assert np.array_equal(got, want[f]), (size, rows, f, np.argwhere(got != want[f])[:8].tolist())


def test_colour_apply_programs_of_both_kinds(monkeypatch):
    rows_env(monkeypatch, 2)
    P = images(36, 17, 2300)
    programs = [JITTER, [("sharpen", 1.9), ("contrast", 1.9)], [("hue", 128), ("equalize", 0), ("sharpen", 0.37)], None]
    t = torch.from_numpy(P).cuda()
    J.colour_apply(t, programs)
    got = t.cpu().numpy()
    for i in range(4):
        assert np.array_equal(got[i], PR.apply(P[i], programs[i])), i


def test_colour_apply_refusals_leave_the_pixels_untouched():
    P = images(36, 17, 2400)
    good = [[("sharpen", 1.9)]] * 4
    t = torch.from_numpy(P).cuda()
    with pytest.raises(J.FormatError):  # (one bad program refuses the call)
        J.colour_apply(t, [good[0], good[1], [("hue", 256)], good[3]])
    with pytest.raises(J.FormatError):
        J.colour_apply(t, [good[0], [(9, 0.0)], None, None])
    with pytest.raises(ValueError):
        J.colour_apply(t, good[:3])
    assert np.array_equal(t.cpu().numpy(), P)
    n = P.size
    flat = torch.zeros(n + 512, dtype=torch.uint8, device="cuda")
    assert flat.data_ptr() % 256 == 0
    flat[4:4 + n] = torch.from_numpy(P.reshape(-1)).cuda()
    off = flat[4:4 + n].view(4, 17, 36, 3)  # (a slice: contiguous, its base 4 bytes behind a 256-byte boundary)
    before = flat.clone()
    with pytest.raises(J.UnsupportedError):
        J.colour_apply(off, good)
    assert torch.equal(flat, before)
    for W, H in ((3, 3), (33, 17)):  # (3 W H % 4 != 0)
        odd = torch.from_numpy(images(W, H, 2401)).cuda()
        keep = odd.clone()
        with pytest.raises(J.UnsupportedError):
            J.colour_apply(odd, good)
        assert torch.equal(odd, keep)
    with pytest.raises(ValueError):
        J.colour_apply(t[:, :, ::2], good)  # (not contiguous)
    with pytest.raises(ValueError):
        J.colour_apply(t.cpu(), good)
    J.colour_apply(t, good)  # (and the call goes on as ever)
    assert np.array_equal(t.cpu().numpy(), np.stack([PR.apply(p, good[0]) for p in P]))


# ---- behind the fixed output size ----

@pytest.mark.parametrize("rows", [0, 1, 2, 3])
@pytest.mark.parametrize("size", [(33, 17), (5, 3), (3, 3), (224, 224)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_batch_u8_bit_exact(monkeypatch, size, rows):
    rows_env(monkeypatch, rows)
    srcs = GC.pick("rgb", len(PROGRAMS))
    outs, path = GC.run(srcs, size, PROGRAMS)
    assert path.endswith("+resize+colour"), path
    changed = 0
    for i, o in enumerate(outs):
        r = GC.resized_u8(srcs[i], size)
        want = want_u8(r, PROGRAMS[i])
        assert o.size == want.size and np.array_equal(o, want.reshape(-1)), (i, size, rows, PROGRAMS[i], np.nonzero(o != want.reshape(-1))[0][:10].tolist())
        changed += not np.array_equal(want, r)
    assert changed >= 5  # (the programs do something)


def test_batch_f32_tensor_with_flips():
    srcs = GC.pick("rgb", len(PROGRAMS))
    fmt, ref_fmt = TN.fmt_of("float32")
    flips = [i % 3 != 1 for i in range(len(srcs))]
    for size in ((33, 17), (5, 3), (224, 224)):
        outs, path = GC.run(srcs, size, PROGRAMS, None, fmt, flips)
        assert path.endswith("+resize+colour+tensor"), path
        for i, o in enumerate(outs):
            u8 = want_u8(GC.resized_u8(srcs[i], size), PROGRAMS[i], flips[i])
            want = T.bits(T.to_tensor(u8, T.table(ref_fmt, 3), False))
            assert o.shape == (3, size[1], size[0]) and np.array_equal(T.bits(o), want), (i, size, PROGRAMS[i], flips[i])


def test_batch_behind_a_warp(monkeypatch):
    """u8 and f32 output behind a bilinear warp, with flips: the programs run in front of it."""
    rows_env(monkeypatch, 3)
    srcs = GC.pick("rgb", len(PROGRAMS))
    fmt, ref_fmt = TN.fmt_of("float32")
    for size in ((33, 17), (5, 3)):
        warps = [None if i % 3 == 0 else WR.rotate_matrix(15.0 * i, size) for i in range(len(srcs))]
        outs, path = GC.run(srcs, size, PROGRAMS, warp="bilinear", warps=warps)
        assert path.endswith("+colour+warp:bilinear"), path
        for i, o in enumerate(outs):
            want = want_u8(GC.resized_u8(srcs[i], size), PROGRAMS[i], False, "bilinear", warps[i])
            assert np.array_equal(o, want.reshape(-1)), (i, size, PROGRAMS[i], warps[i])
        flips = [i % 2 == 0 for i in range(len(srcs))]
        outs, path = GC.run(srcs, size, PROGRAMS, None, fmt, flips, warp="bilinear", warps=warps)
        assert path.endswith("+tensor") and "+colour+warp" in path, path
        for i, o in enumerate(outs):
            u8 = want_u8(GC.resized_u8(srcs[i], size), PROGRAMS[i], flips[i], "bilinear", warps[i])
            assert np.array_equal(T.bits(o), T.bits(T.to_tensor(u8, T.table(ref_fmt, 3), False))), (i, size)


def test_set_colour_behind_a_pending_decode_keeps_the_old_programs():
    """decode; set_colour while that decode is still queued behind torch kernels; decode.  The earlier decode keeps its programs."""
    srcs = GC.pick("rgb", 4)
    size = (33, 17)
    p1, p2 = [PROGRAMS[4], PROGRAMS[2], PROGRAMS[0], PROGRAMS[6]], [PROGRAMS[3], None, PROGRAMS[5], [("hue", 128)]]
    fmt, ref_fmt = TN.fmt_of("float32")
    flips = [False, True, False, True]
    h = StreamHarness("nonblocking")
    b = GC.batch_of(srcs, size, fmt=fmt)
    try:
        GC.upload(b, srcs)
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
                u8 = want_u8(GC.resized_u8(srcs[i], size), programs[i], flips[i])
                want = T.bits(T.to_tensor(u8, T.table(ref_fmt, 3), False)).reshape(-1)
                o = got[k][b.out_offset(i):b.out_offset(i) + b.out_bytes(i)].view(np.uint32)
                assert np.array_equal(o, want), (k, i)
    finally:
        h.close()
        b.close()


def test_batch_refusals_change_nothing():
    srcs = GC.pick("rgb", 3)
    size = (33, 17)
    good = [PROGRAMS[4], None, PROGRAMS[6]]
    b = GC.batch_of(srcs, size)
    try:
        GC.upload(b, srcs)
        b.set_colour(good)
        for bad in ([("hue", 255.5)], [("hue", 256)], [("hue", -1)], [("sharpen", float("nan"))], [("sharpen", 256.5)], [(15, 0.0)], [(18, 0.0)]):
            with pytest.raises(J.FormatError, match="refused"):
                b.set_colour([None, [("sharpen", 1.0)], bad])
        b.decode()
        b.synchronize()
        for i in range(len(srcs)):
            assert np.array_equal(b.download(i), want_u8(GC.resized_u8(srcs[i], size), good[i]).reshape(-1)), i
    finally:
        b.close()


# ---- from JPEG bytes ----

def test_pipeline_fresh_programs_on_a_kept_pipeline(monkeypatch, capfd):
    fs = GP.files()[:8]
    rng = np.random.default_rng(2500)
    ops = [("hue", (0, 1, 43, 128, 255)), ("sharpen", (0.0, 0.37, 1.9, 256.0)), ("brightness", (0.37, 1.9)), ("contrast", (0.37, 1.9)), ("saturation", (0.37, 1.9)),
           ("equalize", (0,))]
    p = J.Pipeline(threads=4)
    try:
        PW._env(monkeypatch, {})
        monkeypatch.setenv("JPGPU_PIPE_TRACE", "1")
        for c in range(3):
            programs = []
            for i in range(len(fs)):
                picks = [ops[int(k)] for k in rng.integers(0, len(ops), int(rng.integers(1, 5)))]
                programs.append([(n, float(v[int(rng.integers(0, len(v)))])) for n, v in picks])
            programs[c] = [J.hue(0.2), J.sharpness(2.0)] if c else [J.sharpness(0.0), J.hue(-0.5)]
            capfd.readouterr()
            out = p.decode(fs, output_size=GP.SIZE, colour=True, colours=programs)
            trace = capfd.readouterr().err
            assert p.kernel_path.endswith("+resize+colour") and ("created" not in trace) == bool(c), (c, p.kernel_path)
            for i, data in enumerate(fs):
                assert not isinstance(out[i], Exception), (c, i, out[i])
                assert np.array_equal(out[i], PR.apply(GP.resized(data), programs[i]).reshape(-1)), (c, i, programs[i])
    finally:
        monkeypatch.delenv("JPGPU_PIPE_TRACE", raising=False)
        p.close()


def test_pipeline_one_bad_program_fails_its_image_alone(monkeypatch):
    PW._env(monkeypatch, {})
    fs = GP.files()[:8]
    good = [("hue", 43), ("sharpen", 1.9)]
    programs = [good, [("hue", 256)], None, [("sharpen", 256.5)], good, [(18, 0.0)], JITTER, [("sharpen", 0.37)]]
    p = J.Pipeline(threads=4)
    try:
        out = p.decode(fs, output_size=GP.SIZE, colour=True, colours=programs)
        for i in (1, 3, 5):
            assert isinstance(out[i], J.FormatError) and "colour" in str(out[i]), (i, out[i])
        for i in (0, 2, 4, 6, 7):
            assert np.array_equal(out[i], PR.apply(GP.resized(fs[i]), programs[i]).reshape(-1)), i
        assert p.timings()["images_ok"] == 5
    finally:
        p.close()
